"""Frame layout helpers: the byte contract between the signal path and the host GUI.

Frame = 16384 bins x (int16 re LE, int16 im LE) = 65536 bytes (imp/sequ2.vhd:153,
scripts/fft_analyzer_gui.py:250-270).  UDP transport = 64 datagrams per frame, payload =
1 index byte + 1024 data bytes (gui.py:48-50, imp/phy_rmii_if.vhd:173,322).
"""
from __future__ import annotations

import math

import numpy as np

FRAME_SIZE_BYTES = 65536
FFT_SIZE = 16384
PACKETS_PER_FRAME = 64
PACKET_DATA_SIZE = FRAME_SIZE_BYTES // PACKETS_PER_FRAME     # 1024
ETHERNET_PAYLOAD_SIZE = PACKET_DATA_SIZE + 1                 # 1025
FS_HZ = 1_000_000.0


def _iq(frame_bytes: bytes):
    if len(frame_bytes) != FRAME_SIZE_BYTES:
        raise ValueError(f"Invalid frame size: {len(frame_bytes)} (expected {FRAME_SIZE_BYTES})")
    a = np.frombuffer(frame_bytes, dtype="<i2").reshape(FFT_SIZE, 2)
    return a[:, 0], a[:, 1]


# ---------------------------------------------------------------------------- what the argument rules below share, each once
def _is_int(v) -> bool:
    """Whether ``v`` is an int: a bool or a float is none."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_number(v) -> bool:
    """Whether ``v`` is an int or a float: a bool or a str is none."""
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _ints(**named) -> tuple:
    """The values as Python ints, in the order given, or ValueError "`name` must be an int" for the first that is none."""
    for name, v in named.items():
        if not _is_int(v):
            raise ValueError(f"{name} must be an int")
    return tuple(int(v) for v in named.values())


def _is_bin_range(lo: int, hi: int) -> bool:
    """Whether [lo, hi) is a range of bins that is not empty."""
    return 0 <= lo < hi <= FFT_SIZE


def _bin_range(lo: int, hi: int) -> None:
    """ValueError unless the ints ``lo`` and ``hi`` are a range of bins."""
    if not _is_bin_range(lo, hi):
        raise ValueError(f"the range must be 0 <= lo < hi <= {FFT_SIZE}")


RANK_FIELDS = {None: None, "peak": 0, "power": 1}      # field -> the float of a (peak, power) record that is the point


def _field(field) -> None:
    """ValueError unless ``field`` is None, 'peak' or 'power'; every rule function looks at it last."""
    if not (field is None or isinstance(field, str)) or field not in RANK_FIELDS:
        raise ValueError("field must be None, 'peak' or 'power'")


def _points(points, field=None) -> np.ndarray:
    """The input of a mirror as a C-contiguous float32 [R, 16384] array: ``points`` itself, or with ``field`` 'peak' or 'power'
    that float of the records [R, 16384, 2]; ValueError on any other dtype or shape.  ``field`` has passed :func:`_field`."""
    points = np.ascontiguousarray(points)
    shape = (FFT_SIZE,) if field is None else (FFT_SIZE, 2)
    if points.dtype != np.float32 or points.ndim != 1 + len(shape) or points.shape[1:] != shape:
        raise ValueError(f"points must be float32 [R, {', '.join(map(str, shape))}]")
    return points if field is None else np.ascontiguousarray(points[..., RANK_FIELDS[field]])


def _key(a: np.ndarray) -> np.ndarray:
    """The keys of float32 values, uint32: the bits with the sign cleared -- +inf above every finite value, a NaN above +inf,
    -0.0 as +0.0, denormals kept."""
    return a.view(np.uint32) & np.uint32(0x7FFFFFFF)


def _threshold_key(threshold) -> int:
    """The key of a threshold common to all rows, or ValueError: a number that is +0.0 .. +inf as a float32."""
    if not _is_number(threshold):
        raise ValueError("threshold must be a number")
    key = int(np.array([threshold], np.float32).view(np.uint32)[0])
    if key > 0x7F800000:
        raise ValueError("threshold must be +0.0 .. +inf: no NaN, no sign bit")
    return key


def decode_mag_16iq_le(frame_bytes: bytes) -> np.ndarray:
    """Same result as gui.py:250-260: float32 sqrt(re^2 + im^2) over all 16384 bins."""
    re, im = _iq(frame_bytes)
    return np.sqrt(re.astype(np.float32) ** 2 + im.astype(np.float32) ** 2)


def marker_of_frame(frame_bytes: bytes, lo: int = 0, hi: int = FFT_SIZE):
    """What the gui shows of a frame cut to the bins [lo, hi) (gui.py:294-305, 415-455): ``(peak_mag float32, peak_bin
    int, band_power int)`` -- np.max and lo + np.argmax of the decoded magnitudes, and the exact integer sum of
    re^2 + im^2.  The host mirror of one sa_marker_q15 record (include/specan.h)."""
    if not _is_bin_range(lo, hi):
        raise ValueError("need 0 <= lo < hi <= 16384")
    mag = decode_mag_16iq_le(frame_bytes)[lo:hi]
    re, im = _iq(frame_bytes)
    power = (re[lo:hi].astype(np.int64) ** 2 + im[lo:hi].astype(np.int64) ** 2).sum()
    return np.float32(mag.max()), lo + int(mag.argmax()), int(power)


TRACE_BUCKETS = (2, 4, 8, 16, 32, 64)


def trace_of_frame(frame_bytes: bytes, bucket: int):
    """A frame reduced to P = 16384 // bucket display points, point j over the bins [j bucket, (j + 1) bucket): ``(peak
    float32 [P], power float32 [P], exact int64 [P])`` -- the largest decoded magnitude of each bucket, the exact integer
    sum of re^2 + im^2 over it rounded once to float32 (numpy's int64 -> float32 conversion rounds to nearest even), and
    that sum itself.  The host mirror of one frame's sa_trace_point_q15 records (include/specan.h, SA_Q15_TRACE_KIND)."""
    if not _is_int(bucket) or int(bucket) not in TRACE_BUCKETS:
        raise ValueError(f"bucket must be one of {TRACE_BUCKETS}")
    bucket = int(bucket)
    peak = decode_mag_16iq_le(frame_bytes).reshape(-1, bucket).max(axis=1)
    re, im = _iq(frame_bytes)
    exact = (re.astype(np.int64) ** 2 + im.astype(np.int64) ** 2).reshape(-1, bucket).sum(axis=1)
    return peak, exact.astype(np.float32), exact


TRACE_GROUPS = (2, 4, 8, 16, 32, 64, 128)


def trace_of_frames(frames_bytes, bucket: int):
    """A group of A = 2, 4, ..., 128 consecutive frames reduced to P = 16384 // bucket display points, point j over the bins
    [j bucket, (j + 1) bucket) of all A frames: ``(peak float32 [P], power float32 [P], exact int64 [P])`` -- the largest of
    the frames' trace_of_frame peaks (max hold), the exact integer sum of re^2 + im^2 over bucket x A bins (at most 2^44)
    rounded once to float32, and that sum itself.  The power is the sum, not the mean: the mean is power / A, exactly.  The
    host mirror of one group's sa_trace_point_q15 records (include/specan.h, SA_Q15_TRACE_AVG_KIND)."""
    frames_bytes = list(frames_bytes)
    if len(frames_bytes) not in TRACE_GROUPS:
        raise ValueError(f"a group is one of {TRACE_GROUPS} frames")
    parts = [trace_of_frame(f, bucket) for f in frames_bytes]
    exact = np.sum([e for _, _, e in parts], axis=0, dtype=np.int64)
    return np.max([p for p, _, _ in parts], axis=0), exact.astype(np.float32), exact


def spectrum_of_frames(frames_bytes):
    """A group of A = 2, 4, ..., 128 consecutive frames reduced bin by bin, at the full resolution of 16384 bins: ``(peak
    float32 [16384], power float32 [16384], exact int64 [16384])`` -- the largest of the frames' decoded magnitudes of each bin
    (max hold), the exact integer sum of re^2 + im^2 over the A frames (at most 2^38) rounded once to float32, and that sum
    itself.  The power is the sum, not the mean: the mean is power / A, exactly.  The host mirror of one row of
    sa_spectra_q15 / sa_fold_iq_q15 (include/specan_ext.h); trace_of_frames is the same over buckets of 2..64 bins."""
    frames_bytes = list(frames_bytes)
    if len(frames_bytes) not in TRACE_GROUPS:
        raise ValueError(f"a group is one of {TRACE_GROUPS} frames")
    peak = np.max([decode_mag_16iq_le(f) for f in frames_bytes], axis=0)
    exact = np.zeros(FFT_SIZE, np.int64)
    for f in frames_bytes:
        re, im = _iq(f)
        exact += re.astype(np.int64) ** 2 + im.astype(np.int64) ** 2
    return peak, exact.astype(np.float32), exact


# A = 2^a, a = 0 .. SA_FOLD_LOG2A_MAX, and W = 2^k, k = 0 .. SA_FOLD_LOG2W_MAX (include/specan_fold.h): the one definition
FOLD_GROUPS = (1, 2, 4, 8, 16, 32, 64, 128)
FOLD_BUCKETS = (1, 2, 4, 8, 16, 32, 64)


def _fold_args(group, bucket) -> tuple:
    """``(group, bucket)`` of the fold as ints, or ValueError: ``group`` one of 1, 2, ..., 128 and ``bucket`` one of 1, 2, ...,
    64 (no bool, no float), not both 1."""
    for name, v, allowed in (("group", group, FOLD_GROUPS), ("bucket", bucket, FOLD_BUCKETS)):
        if not _is_int(v) or int(v) not in allowed:
            raise ValueError(f"{name} must be one of {allowed}")
    if int(group) == 1 and int(bucket) == 1:
        raise ValueError("group = bucket = 1 folds nothing")
    return int(group), int(bucket)


def fold_of_mags(mag, group: int, bucket: int):
    """Float32 magnitudes [B, n] (n = 16384 for the chain's 'mag_full' frames; any multiple of ``bucket`` here) reduced over
    groups of ``group`` = 1, 2, ..., 128 consecutive frames and buckets of ``bucket`` = 1, 2, ..., 64 adjacent bins, not both
    1: ``(peak float32 [B // group, n // bucket], power float32 [same], s64 float64 [same])``.  The numpy mirror of
    sa_fold_mag_f32 (include/specan_fold.h), step for step:

    - peak: the input whose bits with the sign cleared are largest as a uint32, as those bits -- the float maximum of
      non-negative finite data; +inf above every finite value, a NaN above +inf, -0.0 as +0.0, denormals kept;
    - s64: the float64 sum of the exact squares ``float64(m) * float64(m)``, per bin over the frames of the group one after
      the other, ascending, from +0.0 (the explicit loop), then across the bucket's bins by a balanced tree of adjacent
      pairs, ``t[i] = t[2i] + t[2i+1]`` (the explicit halving); power is s64 rounded once to float32 (numpy's cast rounds to
      nearest even, overflows to inf and keeps denormals).  It is the sum: the mean is ``power / (group * bucket)``, exactly."""
    group, bucket = _fold_args(group, bucket)
    mag = np.ascontiguousarray(mag)
    if mag.dtype != np.float32 or mag.ndim != 2 or mag.shape[0] % group or mag.shape[1] % bucket:
        raise ValueError("mag must be float32 [B, n] with B a multiple of group and n a multiple of bucket")
    B, n = mag.shape
    G, P = B // group, n // bucket
    peak = np.ascontiguousarray(_key(mag).reshape(G, group, P, bucket).max(axis=(1, 3))).view(np.float32)
    m = mag.astype(np.float64).reshape(G, group, n)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.zeros((G, n), np.float64)
        for i in range(group):                        # frames ascending, one after the other
            t = t + m[:, i] * m[:, i]
        while t.shape[1] > P:                         # adjacent pairs on the bin index, log2(bucket) levels
            t = t[:, 0::2] + t[:, 1::2]
        power = t.astype(np.float32)
    return peak, power, t


PEAKS_K_MAX = 32


def _peaks_args(k, threshold, lo, hi, min_sep, field) -> tuple:
    """``(k, the threshold's key, lo, hi, min_sep)`` of the peak table as ints, or ValueError: ``k``, ``lo``, ``hi`` and
    ``min_sep`` ints (no bool, no float), ``k`` 1..32, ``threshold`` a number that is +0.0 .. +inf as a float32,
    ``0 <= lo < hi <= 16384``, ``min_sep`` 1..16384; ``field`` None, 'peak' or 'power'."""
    k, lo, hi, min_sep = _ints(k=k, lo=lo, hi=hi, min_sep=min_sep)
    if not 1 <= k <= PEAKS_K_MAX:
        raise ValueError(f"k must be 1..{PEAKS_K_MAX}")
    tkey = _threshold_key(threshold)
    _bin_range(lo, hi)
    if not 1 <= min_sep <= FFT_SIZE:
        raise ValueError(f"min_sep must be 1..{FFT_SIZE}")
    _field(field)
    return k, tkey, lo, hi, min_sep


def peaks_of_rows(points, k: int = 8, threshold: float = 0.0, lo: int = 0, hi: int = FFT_SIZE, min_sep: int = 1):
    """The peak table of float32 ``points`` [R,16384]: ``(mag float32 [R,k], bin int32 [R,k], count int32 [R])``.  The numpy
    mirror of sa_peaks_f32 (include/specan_peaks.h), step for step:

    - key: the float's bits with the sign cleared, as a uint32 -- +inf above every finite value, a NaN above +inf, -0.0 as
      +0.0, denormals kept;
    - candidate: ``lo <= i < hi``, ``u[i] > 0``, ``u[i] >= key(threshold)``, ``u[i] > u[i-1]`` and ``u[i] >= u[i+1]``, the
      neighbours those of the row whether or not they lie in the range, a missing neighbour (i = 0, i = 16383) satisfying its
      condition; count is their number;
    - selection: the candidates sorted by larger key, then lower bin (the sort), walked in that order (the explicit loop): one
      is accepted when it lies ``min_sep`` or more bins from every one accepted before it, until ``k`` are; a candidate that
      was not accepted suppresses nothing;
    - the records in acceptance order, mag the point with its sign cleared; the unused slots are (+0.0, -1).

    The integers are ints (no bool, no float), ``k`` is 1..32, ``threshold`` a number (no bool, no str) that is no NaN and
    not negative (-0.0 included), ``0 <= lo < hi <= 16384``, ``min_sep`` 1..16384: ValueError otherwise, one text per rule
    and in that order (:func:`_peaks_args`, which ``find_peaks`` of the device refuses by too), and on a wrong dtype or
    shape."""
    k, tkey, lo, hi, min_sep = _peaks_args(k, threshold, lo, hi, min_sep, None)
    points = _points(points)
    R = points.shape[0]
    u = _key(points).astype(np.int64)
    left = np.concatenate([np.full((R, 1), -1, np.int64), u[:, :-1]], axis=1)      # below every key: the missing neighbours
    right = np.concatenate([u[:, 1:], np.full((R, 1), -1, np.int64)], axis=1)
    i = np.arange(FFT_SIZE)
    cand = (i >= lo) & (i < hi) & (u > 0) & (u >= tkey) & (u > left) & (u >= right)
    mag = np.zeros((R, k), np.uint32)
    bins = np.full((R, k), -1, np.int32)
    for r in range(R):
        c = np.nonzero(cand[r])[0]
        order = c[np.lexsort((c, -u[r, c]))]          # larger key first, then lower bin
        taken = []
        for p in order:
            if all(abs(int(p) - q) >= min_sep for q in taken):
                taken.append(int(p))
                if len(taken) == k:
                    break
        mag[r, :len(taken)] = u[r, taken]
        bins[r, :len(taken)] = taken
    return mag.view(np.float32), bins, cand.sum(axis=1).astype(np.int32)


RANK_Q_MAX = 8


def _rank_args(ranks, lo, hi, field) -> tuple:
    """``(ranks as a tuple of ints, lo, hi)`` of the order statistics, or ValueError: ``lo`` and ``hi`` ints (no bool, no
    float) with ``0 <= lo < hi <= 16384``, ``ranks`` a sequence of 1..8 ints, each ``0 <= rank < hi - lo``; ``field`` None,
    'peak' or 'power'."""
    lo, hi = _ints(lo=lo, hi=hi)
    _bin_range(lo, hi)
    if isinstance(ranks, (str, bytes)) or not hasattr(ranks, "__len__") or not 1 <= len(ranks) <= RANK_Q_MAX:
        raise ValueError(f"ranks must be a sequence of 1..{RANK_Q_MAX} ints")
    for v in ranks:
        if not _is_int(v) or not 0 <= int(v) < hi - lo:
            raise ValueError(f"a rank must be an int in 0..{hi - lo - 1}")
    _field(field)
    return tuple(int(v) for v in ranks), lo, hi


def ranks_of_rows(points, ranks, lo: int = 0, hi: int = FFT_SIZE, field=None):
    """The order statistics of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the
    records [R,16384,2] -- over the bins [lo, hi): float32 [R, q], one value per row and entry of ``ranks``.  The numpy mirror
    of sa_rank_f32 (include/specan_rank.h):

    - key: the float's bits with the sign cleared, as a uint32 -- +inf above every finite value, a NaN above +inf, -0.0 as
      +0.0, denormals kept;
    - ``s = np.sort`` of the m = hi - lo keys of the slice, ascending; the result is ``s[ranks[j]]`` as float bits: rank 0 is
      the minimum of the range, rank m - 1 its maximum.

    ``ranks`` is a sequence of 1..8 ints, each ``0 <= rank < hi - lo``, in any order, repeats allowed;
    ``0 <= lo < hi <= 16384``; the integers are ints (no bool, no float): ValueError otherwise, and on a wrong dtype or
    shape."""
    ranks, lo, hi = _rank_args(ranks, lo, hi, field)
    s = np.sort(_key(_points(points, field))[:, lo:hi], axis=1)
    return np.ascontiguousarray(s[:, list(ranks)]).view(np.float32)


def rank_of_quantile(q: float, m: int) -> int:
    """The rank of the "lower" quantile ``q`` (0 <= q <= 1) among ``m`` >= 1 sorted values: ``math.floor(q * (m - 1))``,
    the product taken in Python's double arithmetic.  0.0 is the minimum (rank 0), 1.0 the maximum (rank m - 1), 0.5 the
    lower median.  The double product decides, not the decimal one: 0.29 * 100 is 28.999999999999996 in doubles, so
    ``rank_of_quantile(0.29, 101)`` is 28.  ValueError on a q that is no number in [0, 1] (a NaN included) or an m that is no
    int >= 1."""
    if not _is_int(m) or int(m) < 1:
        raise ValueError("m must be an int >= 1")
    if not _is_number(q) or not 0.0 <= float(q) <= 1.0:
        raise ValueError("q must be a number in 0..1")
    return math.floor(float(q) * (int(m) - 1))


HOLD_Q_MAX = 8
HOLD_GROUP_MAX = 128


def _hold_args(ranks, group, field) -> tuple:
    """``(ranks as a tuple of ints, group)`` of the percentile traces, or ValueError: ``group`` an int (no bool, no float) in
    2..128, ``ranks`` a sequence of 1..8 ints, each ``0 <= rank < group``; ``field`` None, 'peak' or 'power'."""
    (group,) = _ints(group=group)
    if not 2 <= group <= HOLD_GROUP_MAX:
        raise ValueError(f"group must be 2..{HOLD_GROUP_MAX}")
    if isinstance(ranks, (str, bytes)) or not hasattr(ranks, "__len__") or not 1 <= len(ranks) <= HOLD_Q_MAX:
        raise ValueError(f"ranks must be a sequence of 1..{HOLD_Q_MAX} ints")
    for v in ranks:
        if not _is_int(v) or not 0 <= int(v) < group:
            raise ValueError(f"a rank must be an int in 0..{group - 1}")
    _field(field)
    return tuple(int(v) for v in ranks), group


def holds_of_rows(points, ranks, group: int, field=None):
    """The percentile traces of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the
    records [R,16384,2] -- over groups of ``group`` consecutive rows: float32 [R // group, q, 16384], one row per group and
    entry of ``ranks``.  The numpy mirror of sa_hold_f32 (include/specan_hold.h):

    - key: the float's bits with the sign cleared, as a uint32 -- +inf above every finite value, a NaN above +inf, -0.0 as
      +0.0, denormals kept;
    - ``s = np.sort`` of the ``group`` keys of a bin in a group, ascending along the frames; the result is ``s[ranks[j]]`` as
      float bits: rank 0 is the min hold, rank ``group - 1`` the max hold, rank ``(group - 1) // 2`` the lower median
      (:func:`rank_of_quantile` gives the rank of a quantile).

    ``group`` is an int in 2..128; ``ranks`` a sequence of 1..8 ints, each ``0 <= rank < group``, in any order, repeats
    allowed; the integers are ints (no bool, no float): ValueError otherwise, on rows that are no multiple of ``group`` and
    on a wrong dtype or shape."""
    ranks, group = _hold_args(ranks, group, field)
    keys = _key(_points(points, field))
    if keys.shape[0] % group:
        raise ValueError(f"the rows ({keys.shape[0]}) must be a multiple of {group}")
    s = np.sort(keys.reshape(keys.shape[0] // group, group, FFT_SIZE), axis=1)
    return np.ascontiguousarray(s[:, list(ranks)]).view(np.float32)


HIST_LEVELS_MAX = 64
HIST_BUCKETS = (1, 2, 4, 8, 16, 32, 64)
HIST_GROUP_MAX = 1 << 24


def _hist_edge_keys(edges) -> np.ndarray:
    """``edges`` as the uint32 keys of 1..63 float32 values, or ValueError: numbers only, each with the sign bit clear and
    no NaN (bits <= 0x7F800000), the keys non-decreasing."""
    if isinstance(edges, (str, bytes)) or not hasattr(edges, "__len__") or not 1 <= len(edges) <= HIST_LEVELS_MAX - 1:
        raise ValueError(f"edges must be a sequence of 1..{HIST_LEVELS_MAX - 1} numbers")
    if not all(_is_number(v) for v in edges):
        raise ValueError("an edge must be a number")
    with np.errstate(over="ignore"):
        keys = np.array([float(v) for v in edges], np.float64).astype(np.float32).view(np.uint32)
    if (keys > 0x7F800000).any():
        raise ValueError("an edge must be +0.0 .. +inf: no NaN, no sign bit")
    if (keys[1:] < keys[:-1]).any():
        raise ValueError("the edges must not decrease")
    return keys


def _hist_args(edges, group, bucket, lo, hi) -> tuple:
    """``(the edges' keys, group, bucket, lo, hi)`` of the level histogram, the last four as ints, or ValueError: ``bucket``,
    ``lo``, ``hi`` and ``group`` ints (no bool, no float), ``group`` 1..2^24 -- or None, all rows, which stays None --
    ``bucket`` one of 1, 2, ..., 64, the edges those of :func:`_hist_edge_keys`, ``0 <= lo < hi <= 16384``, both multiples of
    the bucket."""
    bucket, lo, hi = _ints(bucket=bucket, lo=lo, hi=hi)
    if group is not None:
        group, = _ints(group=group)
        if not 1 <= group <= HIST_GROUP_MAX:
            raise ValueError(f"group must be 1..{HIST_GROUP_MAX}")
    if bucket not in HIST_BUCKETS:
        raise ValueError(f"bucket must be one of {HIST_BUCKETS}")
    edge_keys = _hist_edge_keys(edges)
    if not _is_bin_range(lo, hi) or lo % bucket or hi % bucket:
        raise ValueError(f"the range must be 0 <= lo < hi <= {FFT_SIZE}, both multiples of the bucket")
    return edge_keys, group, bucket, lo, hi


def hist_of_rows(points, edges, group: int = 1, bucket: int = 1, lo: int = 0, hi: int = FFT_SIZE):
    """The level histogram of float32 ``points`` [R,16384]: uint32 [G, C, L], C-contiguous, ``[g, c, l]`` the number of points
    (row, bin) of group g (the rows [g group, (g + 1) group)) and column c (the bins [lo + c bucket, lo + (c + 1) bucket))
    whose level is l.  The numpy mirror of sa_hist_f32 (include/specan_hist.h):

    - key: the float's bits with the sign cleared, as a uint32 -- +inf above every finite value, a NaN above +inf, -0.0 as
      +0.0, denormals kept;
    - level: ``np.searchsorted(edge_keys, keys, side="right")``, the number of edges whose key is not above the point's: a
      value equal to an edge is in the level above it, a NaN in level L - 1, L = len(edges) + 1.

    ``edges`` is a sequence of 1..63 numbers, each +0.0 .. +inf as a float32 and none below the one before; ``group`` is
    1..2^24 and divides R, or None, all rows (G = 1), as for ``level_hist``; ``bucket`` is 1, 2, ..., 64;
    ``0 <= lo < hi <= 16384``, both multiples of ``bucket``; the integers are ints (no bool, no float), looked at in the order bucket, lo, hi, group, before the ranges: ValueError otherwise
    (:func:`_hist_args`, which ``level_hist`` of the device refuses by too), and on a wrong dtype or shape."""
    edge_keys, group, bucket, lo, hi = _hist_args(edges, group, bucket, lo, hi)
    points = _points(points)
    R = points.shape[0]
    if group is None:
        group = max(R, 1)
    if R % group:
        raise ValueError(f"the rows ({R}) must be a multiple of group ({group})")
    G, cols, L = R // group, (hi - lo) // bucket, len(edge_keys) + 1
    keys = _key(points)[:, lo:hi]
    level = np.searchsorted(edge_keys, keys, side="right").reshape(G, group, cols, bucket)
    cell = (np.arange(G).reshape(G, 1, 1, 1) * cols + np.arange(cols).reshape(1, 1, cols, 1)) * L + level
    return np.bincount(cell.ravel(), minlength=G * cols * L).astype(np.uint32).reshape(G, cols, L)


def level_edges_db(top: float, span_db: float, levels: int) -> np.ndarray:
    """``levels - 1`` float32 edges evenly spaced in dB for :func:`hist_of_rows` / sa_hist_f32: the last one is
    ``float32(top)``, the first ``float32(top * 10 ** (-span_db / 20))``, edge j ``top * 10 ** (-span_db / 20 * (1 - j / (levels -
    2)))`` computed in float64 and rounded once.  With ``levels`` = 2 the single edge is ``top``.  A host convenience: the
    edges are an input of the histogram, not part of its definition.  ValueError unless ``top`` is a finite number above 0,
    ``span_db`` a finite number not below 0 and ``levels`` an int in 2..64."""
    if not _is_int(levels) or not 2 <= int(levels) <= HIST_LEVELS_MAX:
        raise ValueError(f"levels must be an int in 2..{HIST_LEVELS_MAX}")
    for name, v in (("top", top), ("span_db", span_db)):
        if not _is_number(v) or not math.isfinite(float(v)):
            raise ValueError(f"{name} must be a finite number")
    if not float(top) > 0.0 or float(span_db) < 0.0:
        raise ValueError("top must be above 0 and span_db not below 0")
    n, top, span_db = int(levels) - 1, float(top), float(span_db)
    if n == 1:
        return np.array([top], np.float32)
    # edge j lies span_db (1 - j / (n - 1)) dB below top: span_db, ..., 0; Python's doubles, each product rounded once
    edges = np.array([top * 10.0 ** (-(span_db * (1.0 - j / (n - 1))) / 20.0) for j in range(n)], np.float64).astype(np.float32)
    edges[-1] = np.float32(top)
    return edges


BANDS_MAX = 16
BANDS_Q_MAX = 4
BANDS_FRAC_MAX = 1.0 - 2.0 ** -32


def _bands_args(bands, fracs, field) -> tuple:
    """``(bands as a tuple of (lo, hi) int pairs, fracs as a tuple of floats)`` of the band power, or ValueError: 1..16 bands,
    each a pair of ints (no bool, no float) with ``0 <= lo < hi <= 16384``; 0..4 fractions, numbers in [0, 1 - 2^-32] (no NaN);
    ``field`` None, 'peak' or 'power'."""
    if isinstance(bands, (str, bytes)) or not hasattr(bands, "__len__") or not 1 <= len(bands) <= BANDS_MAX:
        raise ValueError(f"bands must be a sequence of 1..{BANDS_MAX} (lo, hi) pairs")
    pairs = []
    for b in bands:
        if isinstance(b, (str, bytes)) or not hasattr(b, "__len__") or len(b) != 2:
            raise ValueError("a band must be a (lo, hi) pair")
        if not all(_is_int(v) for v in b):
            raise ValueError("lo and hi of a band must be ints")
        lo, hi = int(b[0]), int(b[1])
        if not _is_bin_range(lo, hi):
            raise ValueError("a band must be 0 <= lo < hi <= 16384")
        pairs.append((lo, hi))
    if isinstance(fracs, (str, bytes)) or not hasattr(fracs, "__len__") or len(fracs) > BANDS_Q_MAX:
        raise ValueError(f"fracs must be a sequence of 0..{BANDS_Q_MAX} numbers")
    for v in fracs:
        if not _is_number(v) or not 0.0 <= float(v) <= BANDS_FRAC_MAX:
            raise ValueError("a fraction must be a number in 0 .. 1 - 2^-32")
    _field(field)
    return tuple(pairs), tuple(float(v) for v in fracs)


def bands_of_rows(points, bands, fracs=(), field=None):
    """The band power of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the records
    [R,16384,2]: ``(power float64 [R, nb], cross int32 [R, nb, nq])``, both C-contiguous.  The numpy mirror of sa_bands_f32
    (include/specan_bands.h), step for step:

    - value: ``a`` is the point with its sign bit cleared, widened to float64 (exact, denormals kept); ``v = a * a`` for the
      magnitudes and for 'peak', ``v = a`` for 'power', which already is a power sum;
    - band (lo, hi): ``w = v`` inside [lo, hi) and +0.0 outside;
    - tree: ``T[0] = w``, ``T[l + 1] = T[l][0::2] + T[l][1::2]`` (the explicit halving, 14 levels); ``power = T[14][0]``,
      not rounded;
    - crossing of the fraction f: ``t = f * power``; from the root with ``E = 0.0`` and ``k = 0``, for l = 13 .. 0 (the
      explicit loop): ``L = T[l][2k]``; where ``E + L >= t`` go left, ``k = 2k``, else ``E = E + L`` and ``k = 2k + 1``; at
      the leaf the result is ``min(max(k, lo), hi - 1)`` where ``E + w[k] >= t`` and -1 otherwise.  A NaN in the band gives -1,
      an all-zero band and a fraction of 0 give lo.

    ``bands`` is a sequence of 1..16 (lo, hi) pairs of ints, ``0 <= lo < hi <= 16384``, in any order, overlapping or repeated;
    ``fracs`` a sequence of 0..4 numbers in [0, 1 - 2^-32], in any order; the integers are ints (no bool, no float):
    ValueError otherwise, and on a wrong dtype or shape."""
    bands, fracs = _bands_args(bands, fracs, field)
    points = _points(points, field)
    R = points.shape[0]
    a = _key(points).view(np.float32).astype(np.float64)
    power = np.zeros((R, len(bands)), np.float64)
    cross = np.zeros((R, len(bands), len(fracs)), np.int32)
    rows = np.arange(R)
    with np.errstate(over="ignore", invalid="ignore"):
        v = a if field == "power" else a * a
        for j, (lo, hi) in enumerate(bands):
            w = np.zeros_like(v)
            w[:, lo:hi] = v[:, lo:hi]
            T = [w]
            while T[-1].shape[1] > 1:                 # adjacent pairs on the bin index, 14 levels
                T.append(T[-1][:, 0::2] + T[-1][:, 1::2])
            S = T[-1][:, 0]
            power[:, j] = S
            for q, f in enumerate(fracs):
                t = f * S
                E = np.zeros(R, np.float64)
                k = np.zeros(R, np.int64)
                for l in range(len(T) - 2, -1, -1):   # 13 .. 0
                    EL = E + T[l][rows, 2 * k]
                    left = EL >= t
                    E = np.where(left, E, EL)
                    k = np.where(left, 2 * k, 2 * k + 1)
                reached = E + w[rows, k] >= t
                cross[:, j, q] = np.where(reached, np.clip(k, lo, hi - 1), -1)
    return power, cross


def channel_bands(center: int, width: int, spacing: int, adjacent: int = 1) -> list:
    """The bands of a channel-power measurement for :func:`bands_of_rows` / sa_bands_f32: the main channel, ``width`` bins
    starting at ``center - width // 2``, then ``adjacent`` channels of the same width on either side, ``spacing`` bins from
    centre to centre, as ``(lo, hi)`` tuples clipped to 0..16384 -- ``[main, lower 1, upper 1, lower 2, upper 2, ...]``.  An
    adjacent channel that lies wholly outside the spectrum is left out.  A host convenience: the bands are an input of the
    call, not part of its definition.  ValueError unless all four are ints (no bool, no float), ``width`` and ``spacing`` are
    1 or more, ``adjacent`` is 0 or more, at most 16 bands result and the main band, clipped, is not empty."""
    center, width, spacing, adjacent = _ints(center=center, width=width, spacing=spacing, adjacent=adjacent)
    if width < 1 or spacing < 1 or adjacent < 0:
        raise ValueError("width and spacing must be 1 or more and adjacent 0 or more")

    def clipped(c):
        lo = c - width // 2
        return max(lo, 0), min(lo + width, FFT_SIZE)

    main = clipped(center)
    if main[0] >= main[1]:
        raise ValueError("the main band is empty")
    out = [main]
    for i in range(1, adjacent + 1):
        for b in (clipped(center - i * spacing), clipped(center + i * spacing)):
            if b[0] < b[1]:
                out.append(b)
    if len(out) > BANDS_MAX:
        raise ValueError(f"more than {BANDS_MAX} bands")
    return out


# sa_mask_row of include/specan_mask.h, 40 bytes
MASK_ROW = np.dtype([("over", "<i4"), ("under", "<i4"), ("first", "<i4"), ("last", "<i4"), ("up_bin", "<i4"), ("lo_bin", "<i4"),
                     ("up_val", "<f4"), ("up_lim", "<f4"), ("lo_val", "<f4"), ("lo_lim", "<f4")])
_MASK_UNITS = {"amplitude": 20.0, "power": 10.0}       # dB = 20 log10 of a ratio of amplitudes, 10 log10 of one of powers


def _mask_args(upper, lower, lo, hi, field) -> tuple:
    """``(lo, hi)`` of the mask test as ints, or ValueError: ``0 <= lo < hi <= 16384`` as ints (no bool, no float), ``field``
    None, 'peak' or 'power', not both limits None.  The limits are only counted here; :func:`_mask_limits` looks at them."""
    lo, hi = _ints(lo=lo, hi=hi)
    _bin_range(lo, hi)
    _field(field)
    if upper is None and lower is None:
        raise ValueError("upper and lower are both None: no limit at all")
    return lo, hi


def _mask_limits(upper, lower) -> tuple:
    """``(upper, lower)`` of the mirror of the mask test, each None or a C-contiguous float32 [16384] array, or ValueError."""
    limits = []
    for name, v in (("upper", upper), ("lower", lower)):
        if v is not None:
            if not isinstance(v, np.ndarray) or v.dtype != np.float32 or v.shape != (FFT_SIZE,):
                raise ValueError(f"{name} must be None or a float32 [16384] array")
            v = np.ascontiguousarray(v)
        limits.append(v)
    return tuple(limits)


def _mask_worst(key, lim, has, up: bool) -> np.ndarray:
    """The bin, or -1, of each row of ``key`` float64 [R, m] that has a limit (``has`` bool [m], ``lim`` float64 [m]) and comes
    first in the order of include/specan_mask.h: the larger (``up``) or smaller key / lim, equal ratios to the lowest bin.  A
    knock-out over adjacent pairs; ``k_i l_j > k_j l_i`` is exact in float64 for values that were float32, and the order is
    total, so the pairing does not matter."""
    R, m = key.shape
    size = 1 << max(m - 1, 0).bit_length()
    k = np.zeros((R, size), np.float64)
    l = np.ones((R, size), np.float64)
    b = np.full((R, size), -1, np.int64)
    k[:, :m] = np.where(has, key, 0.0)
    l[:, :m] = np.where(has, lim, 1.0)
    b[:, :m] = np.where(has, np.arange(m), -1)
    while size > 1:
        kx, ky, lx, ly, bx, by = k[:, 0::2], k[:, 1::2], l[:, 0::2], l[:, 1::2], b[:, 0::2], b[:, 1::2]
        cx, cy = kx * ly, ky * lx                     # keys in [0, +inf], limits finite and above 0: no NaN
        first = ((cx > cy) if up else (cx < cy)) | ((cx == cy) & (bx < by))
        take_x = (by < 0) | ((bx >= 0) & first)
        k, l, b = np.where(take_x, kx, ky), np.where(take_x, lx, ly), np.where(take_x, bx, by)
        size //= 2
    return b[:, 0]


def mask_of_rows(points, upper, lower=None, lo: int = 0, hi: int = FFT_SIZE, field=None):
    """The mask test of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the records
    [R,16384,2] -- against the limit lines ``upper`` and ``lower``, float32 [16384] or None (not both), over the bins [lo, hi):
    ``(records, summary)``, a structured array [R] of dtype MASK_ROW (sa_mask_row) and int32 [4].  The numpy mirror of
    sa_mask_f32 (include/specan_mask.h), exact:

    - ``a`` is the point with its sign bit cleared; nothing is squared.  Bin i has an upper (lower) limit where ``upper[i]``
      (``lower[i]``) is finite and above 0 and ``lo <= i < hi``; any other value leaves a gap;
    - ``over`` counts the bins with an upper limit where ``a > upper`` or a is a NaN, ``under`` those with a lower limit where
      ``a < lower`` or a is a NaN (on the bits as integers: the float32 order of non-negative values); ``first`` and ``last``
      are the lowest and highest bin counted in either, or -1;
    - ``up_bin`` maximises ``a / upper`` as the exact ratio -- cross products in float64, a NaN point standing as +inf, equal
      ratios to the lowest bin -- with ``up_val`` the bits of the point there and ``up_lim`` the limit; ``lo_bin`` minimises
      ``a / lower``, a NaN standing as 0.  Without such a bin the bin is -1 and both floats +0.0;
    - ``summary``: rows with over > 0, rows with under > 0, the first row with either or -1, the last or -1.

    ``0 <= lo < hi <= 16384`` as ints (no bool, no float): ValueError otherwise, and on a wrong dtype or shape."""
    lo, hi = _mask_args(upper, lower, lo, hi, field)
    upper, lower = _mask_limits(upper, lower)
    points = _points(points, field)
    R = points.shape[0]
    a = _key(points)
    nan = a > 0x7F800000
    i = np.arange(FFT_SIZE)
    inside = (i >= lo) & (i < hi)
    rec = np.zeros(R, MASK_ROW)
    outside = np.zeros((R, FFT_SIZE), bool)
    rows = np.arange(R)
    for up, limit, count, names in ((True, upper, "over", ("up_bin", "up_val", "up_lim")),
                                    (False, lower, "under", ("lo_bin", "lo_val", "lo_lim"))):
        rec[names[0]] = -1
        if limit is None:
            continue
        bits = limit.view(np.uint32)
        has = inside & (bits >= 1) & (bits <= 0x7F7FFFFF)             # finite and above 0, denormals included
        out = has & ((a > bits) if up else ((a < bits) | nan))         # as integers: a NaN lies above every limit
        rec[count] = out.sum(axis=1)
        outside |= out
        key = np.where(nan, np.uint32(0x7F800000 if up else 0), a).view(np.float32).astype(np.float64)
        worst = _mask_worst(key[:, lo:hi], limit[lo:hi].astype(np.float64), has[lo:hi], up)
        found = worst >= 0
        at = np.where(found, worst + lo, 0)
        rec[names[0]] = np.where(found, at, -1)
        rec[names[1]] = np.where(found, a[rows, at], np.uint32(0)).astype(np.uint32).view(np.float32)
        rec[names[2]] = np.where(found, limit[at], np.float32(0.0))
    any_out = outside.any(axis=1)
    rec["first"] = np.where(any_out, outside.argmax(axis=1), -1)
    rec["last"] = np.where(any_out, FFT_SIZE - 1 - outside[:, ::-1].argmax(axis=1), -1)
    failed = np.nonzero((rec["over"] > 0) | (rec["under"] > 0))[0]
    summary = np.array([(rec["over"] > 0).sum(), (rec["under"] > 0).sum(), failed[0] if failed.size else -1,
                        failed[-1] if failed.size else -1], np.int32)
    return rec, summary


def limit_line(points, unit: str = "amplitude") -> np.ndarray:
    """A limit line for :func:`mask_of_rows` / sa_mask_f32 from breakpoints: float32 [16384].  ``points`` is a sequence of one
    or more ``(bin, dB)`` pairs, the bins ints in 0..16383 and strictly ascending, the levels finite numbers; consecutive
    breakpoints are joined by a straight line in dB, ``d0 + (d1 - d0) * (i - b0) / (b1 - b0)`` in Python's doubles, and bin i
    gets ``10 ** (dB / 20)`` (``unit='amplitude'``) or ``10 ** (dB / 10)`` (``unit='power'``), computed in float64 and rounded
    once.  Outside the first and last breakpoint the line is +inf: no limit there.  A host convenience: the limits are an
    input of the test, not part of its definition.  ValueError otherwise."""
    if not isinstance(unit, str) or unit not in _MASK_UNITS:
        raise ValueError("unit must be 'amplitude' or 'power'")
    if isinstance(points, (str, bytes)) or not hasattr(points, "__len__") or len(points) < 1:
        raise ValueError("points must be a sequence of one or more (bin, dB) pairs")
    pairs = []
    for p in points:
        if isinstance(p, (str, bytes)) or not hasattr(p, "__len__") or len(p) != 2:
            raise ValueError("a breakpoint must be a (bin, dB) pair")
        b, d = p
        if not _is_int(b) or not 0 <= int(b) < FFT_SIZE:
            raise ValueError("a breakpoint's bin must be an int in 0..16383")
        if not _is_number(d) or not math.isfinite(float(d)):
            raise ValueError("a breakpoint's level must be a finite number of dB")
        if pairs and int(b) <= pairs[-1][0]:
            raise ValueError("the breakpoints' bins must ascend strictly")
        pairs.append((int(b), float(d)))
    div = _MASK_UNITS[unit]
    db = np.full(FFT_SIZE, np.inf, np.float64)
    for (b0, d0), (b1, d1) in zip(pairs, pairs[1:]):
        for i in range(b0, b1):
            db[i] = d0 + (d1 - d0) * (i - b0) / (b1 - b0)
    db[pairs[-1][0]] = pairs[-1][1]
    with np.errstate(over="ignore"):
        return np.array([10.0 ** (d / div) if math.isfinite(d) else math.inf for d in db], np.float64).astype(np.float32)


def mask_from_trace(trace, margin_db: float, widen: int, unit: str = "amplitude") -> np.ndarray:
    """The usual "auto mask" from a known-good spectrum, an upper limit for :func:`mask_of_rows` / sa_mask_f32: float32
    [16384], bin i the largest of ``|trace|`` over the bins ``i - widen .. i + widen`` (those of the row) times ``10 **
    (margin_db / 20)`` (``unit='amplitude'``) or ``10 ** (margin_db / 10)`` (``unit='power'``), the product taken in float64
    and rounded once.  With ``widen`` 0 and a margin of 0 it is ``|trace|``; with a margin of 0 or more the trace passes its
    own mask (the rounding of a product by a factor of 1 or more never goes below the float32 it started from).  Where the
    window's largest value is 0 or a NaN the result is no limit.  ValueError unless ``trace`` is float32 [16384],
    ``margin_db`` a finite number and ``widen`` an int in 0..16384."""
    if not isinstance(unit, str) or unit not in _MASK_UNITS:
        raise ValueError("unit must be 'amplitude' or 'power'")
    if not _is_int(widen) or not 0 <= int(widen) <= FFT_SIZE:
        raise ValueError("widen must be an int in 0..16384")
    if not _is_number(margin_db) or not math.isfinite(float(margin_db)):
        raise ValueError("margin_db must be a finite number")
    if not isinstance(trace, np.ndarray) or trace.dtype != np.float32 or trace.shape != (FFT_SIZE,):
        raise ValueError("trace must be a float32 [16384] array")
    w = int(widen)
    a = _key(np.ascontiguousarray(trace)).view(np.float32)
    L = 2 * w + 1
    m = np.concatenate([np.zeros(w, np.float32), a, np.zeros(w, np.float32)])
    span = 1
    while 2 * span <= L:                              # m[i] = max of the padded row over [i, i + span)
        m = np.maximum(m[:-span], m[span:])
        span *= 2
    widened = np.maximum(m[:FFT_SIZE], m[L - span:L - span + FFT_SIZE])
    with np.errstate(over="ignore"):
        return (widened.astype(np.float64) * 10.0 ** (float(margin_db) / _MASK_UNITS[unit])).astype(np.float32)


def mask_margin_db(records, unit: str = "amplitude") -> tuple:
    """``(upper, lower)`` float64 [R]: the margins in dB of the worst bins of mask records (the MASK_ROW array of
    :func:`mask_of_rows`, or the device's records viewed with that dtype): ``20 log10(up_val / up_lim)`` and ``20 log10(lo_val /
    lo_lim)``, 10 log10 with ``unit='power'``.  A row is over its upper limit where the first is above 0, under its lower
    limit where the second is below 0.  A NaN point stands as in the test, +inf above and -inf below; a row without a
    limited bin gives a NaN."""
    if not isinstance(unit, str) or unit not in _MASK_UNITS:
        raise ValueError("unit must be 'amplitude' or 'power'")
    records = np.asarray(records)
    if records.dtype != MASK_ROW:
        raise ValueError("records must have the dtype MASK_ROW")
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for up, b, v, l in ((True, "up_bin", "up_val", "up_lim"), (False, "lo_bin", "lo_val", "lo_lim")):
            val = records[v].astype(np.float64)
            val = np.where(np.isnan(val), np.inf if up else 0.0, val)
            db = _MASK_UNITS[unit] * np.log10(val / records[l].astype(np.float64))
            out.append(np.where(records[b] >= 0, db, np.nan))
    return out[0], out[1]


HARM_MAX = 10
HARM_SPAN_MAX = 64
HARM_TOP_MAX = FFT_SIZE // 2 + 1
# sa_harm_row of include/specan_harm.h: the record of one row, 168 bytes without a gap
HARM_ROW = np.dtype([("power", "<f8", (HARM_MAX,)), ("dist", "<f8"), ("nad", "<f8"), ("noise", "<f8"), ("bin", "<i4", (HARM_MAX,)),
                     ("fund", "<f4"), ("spur", "<f4"), ("nonharm", "<f4"), ("spur_bin", "<i4"), ("nonharm_bin", "<i4"),
                     ("n_noise", "<i4")])


def _harm_args(order, span, lo, hi, fund, dc, top, field) -> tuple:
    """``(dc, top, lo, hi, fund, span, order)`` of the harmonic analysis as ints, the defaults filled in (``dc = span + 1``,
    ``lo = dc``, ``hi = top``, ``fund = -1`` for a search), or ValueError: every one an int (no bool, no float),
    ``0 <= dc < top <= 8193``, ``dc <= lo < hi <= top``, ``fund`` None, -1 or in [dc, top), ``span`` 0..64, ``order`` 1..10;
    ``field`` None, 'peak' or 'power'."""
    given = dict(order=order, span=span, lo=lo, hi=hi, fund=fund, dc=dc, top=top)
    _ints(**{name: v for name, v in given.items() if v is not None or name in ("order", "span", "top")})
    order, span, top = int(order), int(span), int(top)
    if not 0 <= span <= HARM_SPAN_MAX:
        raise ValueError(f"span must be 0..{HARM_SPAN_MAX}")
    if not 1 <= order <= HARM_MAX:
        raise ValueError(f"order must be 1..{HARM_MAX}")
    dc = span + 1 if dc is None else int(dc)
    if not 0 <= dc < top <= HARM_TOP_MAX:
        raise ValueError(f"the analysed bins must be 0 <= dc < top <= {HARM_TOP_MAX}")
    lo = dc if lo is None else int(lo)
    hi = top if hi is None else int(hi)
    if not dc <= lo < hi <= top:
        raise ValueError("the search range must be dc <= lo < hi <= top")
    fund = -1 if fund is None else int(fund)
    if fund != -1 and not dc <= fund < top:
        raise ValueError("fund must be None, -1 or a bin in [dc, top)")
    _field(field)
    return dc, top, lo, hi, fund, span, order


def harm_alias_bins(k1, order: int) -> np.ndarray:
    """int64 [..., order]: the bins harmonics 1..``order`` of the fundamental bins ``k1`` alias to in a real spectrum of 16384
    points: ``m = (h * k1) mod 16384``, folded about 8192."""
    m = (np.asarray(k1, np.int64)[..., None] * np.arange(1, int(order) + 1)) % FFT_SIZE
    return np.where(m <= FFT_SIZE // 2, m, FFT_SIZE - m)


def _tree_sum(w: np.ndarray) -> np.ndarray:
    """The balanced tree of adjacent pairs over the last axis (a power of two long), by explicit halving."""
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    return w[..., 0]


def harm_of_rows(points, order: int = 5, span: int = 3, lo=None, hi=None, fund=None, dc=None, top: int = HARM_TOP_MAX, field=None):
    """The harmonic analysis of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the
    records [R,16384,2]: a HARM_ROW array [R].  The numpy mirror of sa_harm_f32 (include/specan_harm.h), step for step:

    - key: the point's bits with the sign cleared, compared as integers (a NaN above +inf, -0.0 as +0.0, denormals kept);
      value: that float widened to float64, ``v = a * a`` for the magnitudes and for 'peak', ``v = a`` for 'power';
    - fundamental ``k1``: ``fund`` where given, else ``np.argmax`` of the int64 keys of [lo, hi) -- the first of equal maxima;
    - harmonic h = 2..order aliases to ``m = (h * k1) mod 16384``, ``k = m if m <= 8192 else 16384 - m``;
    - the band of a tone at bin k is ``[max(k - span, dc), min(k + span + 1, top))``, possibly empty; ``F`` is that of k1,
      ``B_h`` that of k_h less F, ``U`` the union of the B_h, ``A = [dc, top)``;
    - a sum over a set: ``w = v`` inside it and +0.0 outside, ``T[0] = w``, ``T[l + 1] = T[l][0::2] + T[l][1::2]`` (the
      explicit halving, 14 levels), not rounded.  ``power[0]`` is the sum over F and ``power[h - 1]`` over B_h (+0.0 in the
      unused slots), ``dist`` over U, ``nad`` over A - F, ``noise`` over A - F - U: five kinds of tree, each summed on its own;
    - ``fund`` is the point at k1 (sign cleared); ``spur, spur_bin`` the largest key of A - F and its bin, ``nonharm,
      nonharm_bin`` that of A - F - U, first of equal maxima, (+0.0, -1) for an empty set; ``n_noise`` the bins of A - F - U;
      ``bin`` is k1, k_2 .. k_order, -1 in the unused slots.

    Defaults: ``dc = span + 1``, ``lo = dc``, ``hi = top``.  The integers are ints (no bool, no float), within the ranges of
    the header: ValueError otherwise, and on a wrong dtype or shape."""
    dc, top, lo, hi, fund, span, order = _harm_args(order, span, lo, hi, fund, dc, top, field)
    points = _points(points, field)
    R = points.shape[0]
    bits = _key(points)
    keys = bits.astype(np.int64)
    a = bits.view(np.float32).astype(np.float64)
    rec = np.zeros(R, HARM_ROW)
    rec["bin"] = -1
    rows = np.arange(R)
    idx = np.arange(FFT_SIZE)
    k1 = np.full(R, fund, np.int64) if fund >= 0 else lo + np.argmax(keys[:, lo:hi], axis=1)
    k = harm_alias_bins(k1, order)                                 # [R, order]; k[:, 0] is k1
    rec["bin"][:, :order] = k
    rec["fund"] = bits[rows, k1].view(np.float32)
    b_lo, b_hi = np.maximum(k - span, dc), np.minimum(k + span + 1, top)
    band = (idx >= b_lo[..., None]) & (idx < b_hi[..., None])      # [R, order, 16384]
    F = band[:, 0]
    A = np.broadcast_to((idx >= dc) & (idx < top), F.shape)
    U = band[:, 1:].any(axis=1) & ~F
    rest = A & ~F
    noise = rest & ~U

    def largest(member):
        masked = np.where(member, keys, -1)
        at = np.argmax(masked, axis=1)
        some = masked[rows, at] >= 0
        return np.where(some, bits[rows, at], 0).astype(np.uint32).view(np.float32), np.where(some, at, -1)

    with np.errstate(over="ignore", invalid="ignore"):
        v = a if field == "power" else a * a
        rec["power"][:, 0] = _tree_sum(np.where(F, v, 0.0))
        for h in range(1, order):
            rec["power"][:, h] = _tree_sum(np.where(band[:, h] & ~F, v, 0.0))
        rec["dist"] = _tree_sum(np.where(U, v, 0.0))
        rec["nad"] = _tree_sum(np.where(rest, v, 0.0))
        rec["noise"] = _tree_sum(np.where(noise, v, 0.0))
    rec["spur"], rec["spur_bin"] = largest(rest)
    rec["nonharm"], rec["nonharm_bin"] = largest(noise)
    rec["n_noise"] = noise.sum(axis=1)
    return rec


def harm_metrics(records, unit: str = "amplitude") -> dict:
    """The dynamic figures of harmonic records (the HARM_ROW array of :func:`harm_of_rows`, or the device's records viewed with
    that dtype), float64 host arithmetic, as a dict of arrays [R] (``hd_dbc`` [R, 10]):

    - ``sfdr_dbc``: ``20 log10(fund / spur)``, ``10 log10`` with ``unit='power'`` (the points of ``field='power'``);
      ``sfdr_nonharm_dbc`` the same against ``nonharm``;
    - ``thd_dbc``: ``10 log10(dist / power[0])``; ``hd_dbc[:, h - 1]``: ``10 log10(power[h - 1] / power[0])`` of harmonic h,
      0 in column 0, NaN in the unused slots;
    - ``sinad_db``: ``10 log10(power[0] / nad)``; ``snr_db``: ``10 log10(power[0] / noise)``; ``enob``: ``(sinad_db - 1.76) /
      6.02``.

    The sums are powers whatever the unit of the points.  A ratio with a zero numerator is -inf and with a zero denominator
    +inf; 0 / 0 and a NaN give a NaN."""
    if not isinstance(unit, str) or unit not in _MASK_UNITS:
        raise ValueError("unit must be 'amplitude' or 'power'")
    records = np.asarray(records)
    if records.dtype != HARM_ROW:
        raise ValueError("records must have the dtype HARM_ROW")
    p1 = records["power"][..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        def db(num, den, scale=10.0):
            return scale * np.log10(np.asarray(num, np.float64) / np.asarray(den, np.float64))

        hd = db(records["power"], p1[..., None])
        hd = np.where(records["bin"] >= 0, hd, np.nan)
        sinad = db(p1, records["nad"])
        return {
            "sfdr_dbc": db(records["fund"], records["spur"], _MASK_UNITS[unit]),
            "sfdr_nonharm_dbc": db(records["fund"], records["nonharm"], _MASK_UNITS[unit]),
            "thd_dbc": db(records["dist"], p1),
            "hd_dbc": hd,
            "sinad_db": sinad,
            "snr_db": db(p1, records["noise"]),
            "enob": (sinad - 1.76) / 6.02,
        }


SIGNALS_K_MAX = 32
SIGNALS_GAP_MAX = FFT_SIZE - 1
# sa_signal of include/specan_signals.h: one record of the signal list, 24 bytes without a gap
SIGNAL = np.dtype([("start", "<i4"), ("stop", "<i4"), ("peak", "<f4"), ("peak_bin", "<i4"), ("power", "<f8")])


def _signals_args(k, lo, hi, gap, min_width, field) -> tuple:
    """``(k, lo, hi, gap, min_width)`` of the signal list as ints, or ValueError: every one an int (no bool, no float), ``k``
    1..32, ``0 <= lo < hi <= 16384``, ``gap`` 0..16383, ``min_width`` 1..16384; ``field`` None, 'peak' or 'power'."""
    k, lo, hi, gap, min_width = _ints(k=k, lo=lo, hi=hi, gap=gap, min_width=min_width)
    if not 1 <= k <= SIGNALS_K_MAX:
        raise ValueError(f"k must be 1..{SIGNALS_K_MAX}")
    _bin_range(lo, hi)
    if not 0 <= gap <= SIGNALS_GAP_MAX:
        raise ValueError(f"gap must be 0..{SIGNALS_GAP_MAX}")
    if not 1 <= min_width <= FFT_SIZE:
        raise ValueError(f"min_width must be 1..{FFT_SIZE}")
    _field(field)
    return k, lo, hi, gap, min_width


def signals_of_rows(points, k: int = 16, threshold=0.0, lo: int = 0, hi: int = FFT_SIZE, gap: int = 0, min_width: int = 1,
                    field=None):
    """The signal list of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the records
    [R,16384,2]: ``(records SIGNAL [R, k], stats int32 [R, 3])``.  The numpy mirror of sa_signals_f32
    (include/specan_signals.h), step for step:

    - key: the point's bits with the sign cleared, compared as integers (a NaN above +inf, -0.0 as +0.0, denormals kept);
    - threshold: a number, +0.0 .. +inf, whose key is that of every row, or a float32 array [R] keyed like the points: a
      negative value counts by its magnitude, a NaN passes only NaN points;
    - on: ``lo <= i < hi``, ``u[i] > 0`` and ``u[i] >= T_r``;
    - closing: ``p[i]`` is the last on bin at or below i (a running maximum) and ``n[i]`` the first at or above it (a running
      minimum from the right); an off bin with both is bridged where ``n[i] - p[i] - 1 <= gap``;
    - segments: the runs of ``on | bridged`` (the differences of the mask), kept where ``stop - start >= min_width``; the
      records are the first ``k`` kept, ``peak`` the largest key of [start, stop) as a float with ``peak_bin`` the first such
      bin, ``power`` the balanced tree of adjacent pairs of :func:`bands_of_rows` over the band [start, stop); the unused slots
      are (-1, -1, +0.0, -1, +0.0);
    - stats: (kept segments before the truncation to k, on bins, the bins of all kept segments).

    ``k`` is 1..32, ``0 <= lo < hi <= 16384``, ``gap`` 0..16383, ``min_width`` 1..16384, the integers ints (no bool, no
    float): ValueError otherwise, and on a wrong dtype or shape."""
    k, lo, hi, gap, min_width = _signals_args(k, lo, hi, gap, min_width, field)
    points = _points(points, field)
    R = points.shape[0]
    if isinstance(threshold, np.ndarray):
        if threshold.dtype != np.float32 or threshold.shape != (R,):
            raise ValueError(f"a threshold per row must be float32 [{R}]")
        T = _key(np.ascontiguousarray(threshold)).astype(np.int64)
    else:
        T = np.full(R, _threshold_key(threshold), np.int64)
    bits = _key(points)
    keys = bits.astype(np.int64)
    a = bits.view(np.float32).astype(np.float64)
    idx = np.arange(FFT_SIZE)
    on = (idx >= lo) & (idx < hi) & (keys > 0) & (keys >= T[:, None])
    prev = np.maximum.accumulate(np.where(on, idx, -1), axis=1)
    nxt = np.minimum.accumulate(np.where(on, idx, 2 * FFT_SIZE)[:, ::-1], axis=1)[:, ::-1]
    closed = on | ((prev >= 0) & (nxt < 2 * FFT_SIZE) & (nxt - prev - 1 <= gap))
    edges = np.diff(closed.astype(np.int8), axis=1, prepend=0, append=0)              # [R, 16385]: +1 at a start, -1 at a stop
    rec = np.zeros((R, k), SIGNAL)
    rec["start"] = rec["stop"] = rec["peak_bin"] = -1
    stats = np.zeros((R, 3), np.int32)
    stats[:, 1] = on.sum(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        v = a if field == "power" else a * a
        for r in range(R):
            start, stop = np.nonzero(edges[r] == 1)[0], np.nonzero(edges[r] == -1)[0]
            keep = stop - start >= min_width
            start, stop = start[keep], stop[keep]
            stats[r, 0], stats[r, 2] = len(start), (stop - start).sum()
            m = min(len(start), k)
            if m == 0:
                continue
            inside = (idx >= start[:m, None]) & (idx < stop[:m, None])                # [m, 16384]
            at = np.argmax(np.where(inside, keys[r], -1), axis=1)
            rec["start"][r, :m], rec["stop"][r, :m] = start[:m], stop[:m]
            rec["peak"][r, :m], rec["peak_bin"][r, :m] = bits[r, at].view(np.float32), at
            rec["power"][r, :m] = _tree_sum(np.where(inside, v[r], 0.0))
    return rec, stats


CFAR_TRAINS = (1, 2, 4, 8, 16, 32, 64)
CFAR_GUARD_MAX = 64
CFAR_MODES = {"ca": 0, "go": 1, "so": 2}               # mode -> SA_CFAR_MODE_* of include/specan_cfar.h
CFAR_OUTPUTS = {"ratio": 0, "floor": 1}                # what -> SA_CFAR_OUT_*


def _cfar_args(train, guard, mode, what, lo, hi, field) -> tuple:
    """``(log2_train, guard, mode code, what code, lo, hi)`` of the CFAR normalisation, or ValueError: ``train``, ``guard``,
    ``lo`` and ``hi`` ints (no bool, no float), ``train`` one of 1, 2, 4, ..., 64, ``guard`` 0..64, ``mode`` 'ca', 'go' or
    'so', ``what`` 'ratio' or 'floor', ``0 <= lo < hi <= 16384`` with ``hi - lo >= 2 * guard + 2``; ``field`` None, 'peak' or
    'power'."""
    train, guard, lo, hi = _ints(train=train, guard=guard, lo=lo, hi=hi)
    if train not in CFAR_TRAINS:
        raise ValueError(f"train must be one of {CFAR_TRAINS}")
    if not 0 <= guard <= CFAR_GUARD_MAX:
        raise ValueError(f"guard must be 0..{CFAR_GUARD_MAX}")
    if not isinstance(mode, str) or mode not in CFAR_MODES:
        raise ValueError("mode must be 'ca', 'go' or 'so'")
    if not isinstance(what, str) or what not in CFAR_OUTPUTS:
        raise ValueError("what must be 'ratio' or 'floor'")
    _bin_range(lo, hi)
    if hi - lo < 2 * guard + 2:
        raise ValueError("the range must hold 2 * guard + 2 bins or more")
    _field(field)
    return train.bit_length() - 1, guard, CFAR_MODES[mode], CFAR_OUTPUTS[what], lo, hi


def cfar_alpha(pfa: float, n: int) -> float:
    """The ratio threshold ``n * (pfa ** (-1 / n) - 1)`` of a cell-averaging detector over ``n`` training cells of
    exponentially distributed power (the squared magnitude of complex Gaussian noise) at the false-alarm probability
    ``pfa`` per bin: a bin of noise alone exceeds ``alpha`` times the mean of its n cells with that probability.  For
    ``cfar_of_rows(..., mode='ca', what='ratio')`` n is 2 * train.  It applies to single frames: the sum of a ``group`` of
    frames is gamma, not exponentially, distributed, and its threshold is lower.  ``0 < pfa < 1`` and ``n`` an int of 1 or
    more: ValueError otherwise."""
    if not _is_int(n) or n < 1:
        raise ValueError("n must be an int of 1 or more")
    if not _is_number(pfa) or not 0.0 < pfa < 1.0:
        raise ValueError("pfa must be a number above 0 and below 1")
    return int(n) * (float(pfa) ** (-1.0 / int(n)) - 1.0)


def cfar_of_rows(points, train: int = 16, guard: int = 2, mode: str = "ca", what: str = "ratio", lo: int = 0,
                 hi: int = FFT_SIZE, field=None) -> np.ndarray:
    """The CFAR normalisation of float32 ``points`` [R,16384] -- or, with ``field`` 'peak' or 'power', of that float of the
    records [R,16384,2]: float32 [R,16384], every bin of ``[lo, hi)`` over the mean power of its training cells
    (``what='ratio'``) or that mean itself (``'floor'``), +0.0 outside the range.  The numpy mirror of sa_cfar_f32
    (include/specan_cfar.h), step for step:

    - point: ``a`` the point with its sign cleared as a float64, ``v = a * a``, or ``v = a`` with ``field='power'``;
    - cells: ``c[j] = v[j]`` inside ``[lo, hi)`` and +0.0 for every other j, on a row padded with zeros on either side;
    - window sums by doubling: ``W = W[:, :-h] + W[:, h:]`` for h = 1, 2, ..., train / 2: ``W[j]`` is the balanced pair tree
      over the cells j .. j + train - 1;
    - sides of bin i: ``L = W[i - guard - train]`` and ``R = W[i + guard + 1]`` with ``nL`` and ``nR`` their cells inside
      ``[lo, hi)``;
    - mode: 'ca' takes ``S = L + R`` and ``n = nL + nR``; 'go' the side with the larger mean and 'so' the one with the
      smaller: the left with ``nR == 0``, the right with ``nL == 0``, otherwise the left where ``L * nR >= R * nL`` ('go')
      or ``<=`` ('so');
    - output: ``float32((v * n) / S)`` or ``float32(S / n)``; 0x7FC00000 where L or R is a NaN or, for the ratio, the point
      is one; with ``S == 0`` the ratio is +0.0 where v is 0 and +inf otherwise and the floor +0.0; a quotient that is a
      NaN is 0x7FC00000.

    ``train`` is 1, 2, 4, ..., 64, ``guard`` 0..64, ``0 <= lo < hi <= 16384`` with ``hi - lo >= 2 * guard + 2``, the integers
    ints (no bool, no float): ValueError otherwise, and on a wrong dtype or shape."""
    t, G, mode, what, lo, hi = _cfar_args(train, guard, mode, what, lo, hi, field)
    T = 1 << t
    points = _points(points, field)
    R = points.shape[0]
    a = _key(points).view(np.float32).astype(np.float64)
    idx = np.arange(FFT_SIZE)
    pad = G + T                                                            # W is wanted for j = -pad .. 16383 + G + 1
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = a if field == "power" else a * a
        W = np.zeros((R, pad + FFT_SIZE + pad + T), np.float64)           # column e is cell e - pad
        W[:, pad + lo:pad + hi] = v[:, lo:hi]
        h = 1
        while h < T:
            W = W[:, :-h] + W[:, h:]
            h *= 2
        L, Rt = W[:, idx], W[:, idx + pad + G + 1]                         # W[i - G - T] and W[i + G + 1]
        nL = np.maximum(0, np.minimum(idx - G, hi) - np.maximum(idx - G - T, lo))
        nR = np.maximum(0, np.minimum(idx + G + 1 + T, hi) - np.maximum(idx + G + 1, lo))
        if mode == 0:
            S, n = L + Rt, np.broadcast_to(nL + nR, L.shape)
        else:
            pl, pr = L * nR.astype(np.float64), Rt * nL.astype(np.float64)
            left = (pl >= pr) if mode == 1 else (pl <= pr)
            left = np.where(nR == 0, True, np.where(nL == 0, False, left))
            S, n = np.where(left, L, Rt), np.where(left, nL, nR)
        dn = n.astype(np.float64)
        q = (v * dn) / S if what == 0 else S / dn
        bits = q.astype(np.float32).view(np.uint32).copy()
        bits[np.isnan(q)] = 0x7FC00000
        zero = S == 0
        bits[zero] = np.where(v[zero] != 0, 0x7F800000, 0) if what == 0 else 0
        nan = np.isnan(L) | np.isnan(Rt)
        if what == 0:
            nan |= np.isnan(v)
        bits[nan] = 0x7FC00000
    bits[:, :lo] = 0
    bits[:, hi:] = 0
    return bits.view(np.float32)


def decode_iq_components(frame_bytes: bytes):
    """Same result as gui.py:262-270: (re, im) as float32 arrays."""
    re, im = _iq(frame_bytes)
    return re.astype(np.float32), im.astype(np.float32)


def frequency_axis_khz(n_bins: int = FFT_SIZE) -> np.ndarray:
    """Bin k -> k*FS/N in kHz over all N bins (gui.py:297)."""
    return np.arange(n_bins, dtype=np.float32) * (FS_HZ / FFT_SIZE) / 1e3


def bin_range_from_permille(start: float, end: float, n_bins: int = FFT_SIZE) -> tuple[int, int]:
    """The gui's frequency range (per mille of the N bins, gui.py:294-305) as the bin range [lo, hi) it slices.

    Both ends are truncated toward zero, then lo is clamped to [0, N-1] and hi to [lo+1, N]: the slice is never empty.
    (lo, hi) is what SpectrumChain.set_marker_range takes, and frequency_axis_khz()[peak_bin] the gui's peak_frequency."""
    lo = int(float(start) * n_bins / 1000.0)
    hi = int(float(end) * n_bins / 1000.0)
    lo = min(max(lo, 0), n_bins - 1)
    hi = max(min(hi, n_bins), lo + 1)
    return lo, hi


def frame_to_udp_payloads(frame_bytes: bytes) -> list[bytes]:
    """Cut a frame into the 64 datagram payloads the FPGA MAC sends: index byte 0..63 followed by
    1024 data bytes (consumed by MultiPacketAssembler.add, gui.py:318-339)."""
    if len(frame_bytes) != FRAME_SIZE_BYTES:
        raise ValueError("frame must be 65536 bytes")
    return [bytes([i]) + frame_bytes[i * PACKET_DATA_SIZE:(i + 1) * PACKET_DATA_SIZE]
            for i in range(PACKETS_PER_FRAME)]
