"""Shared by tests/test_drawn_cases_cpu.py (the guard) and tests/test_gpu_f32_drawn.py (a plain module, like offset_cases.py: no
fixtures, importable without torch and without a GPU): rows and arguments DRAWN for the nine handle-free reduction libraries,
the numpy mirror of each call, the comparison of a result with the mirror's, the kernel instantiations a draw launches and
the kinds of outcome the draws must reach.

The rows and argument tuples of tests/test_gpu_f32_x.py were placed by hand at the seams their author knew about.  Here they
are drawn: D draws per library, every one from ``numpy.random.default_rng([SEED, index of the library])``, so that one
library's draws do not move when another's generator changes.  A draw is (index, pts float32 [R, 16384], field, kw): ``kw``
is what the mirror and the SpectrumChain method take alike, a limit line of the mask test and a threshold per row of the
signal list as numpy arrays that the GPU tests move to the device.

Rows.  Each row comes from a family that is itself drawn: (a) exp(U(-20, 20)); (b) |N(0, 1)| with a few tones of 20 to 2000;
(c) the integers 0..3 (plateaus and ties everywhere); (d) a zero row with 1..200 spikes; (e) exp(U(-3, 3)) with about 0.2 % of
the points +inf, -0.0, a float32 denormal or negative; (f) a constant 0, 1 or 3.5; (g) exp(U(-3, 3)) with one NaN.  Every header
defines the result for a NaN (include/specan_x.h: a NaN's key lies above +inf's; the sums and quotients it enters are NaNs, a
crossing -1), so (g) is drawn for all nine.  R is 1..8; for the histogram a multiple of the group, and in a few draws 64..130
rows in one group over a narrow range, which takes the sliced form (hist_slices).

Integers.  20 % an end of the valid range, 30 % at or one off a multiple of an ownership size of that library's kernel (SIZES:
the 4-bin quads, 2-bin record units, 64-bin mask words, 128- and 256-bin wave tiles and 512- and 1024-bin rounds of the
kernels' header comments, the 2048-bin tiles and 128-cell halo of cfar, kHistTile), the rest uniform over the range.

What was kept.  SEED = 2610 reached every kind of KINDS in 3 draws or more with these weights, which are the generator's and
not the threshold's: the uniform part of ``min_sep``, ``gap`` and ``min_width`` is uniform in the logarithm (uniform over
1..16384 makes almost every one so wide that one peak or no segment is left); a peak threshold lies above every finite point
of the rows in 15 % of the draws; 15 % of the ranges are at most 300 bins wider than the least width; the cfar range ends
inside the first tile in 15 % and inside the last in 15 % of the draws; 8 % of the histogram's draws are the long group.
"""
import collections
import functools

import numpy as np

import reduction_libraries as rl
from conftest import N
from reduction_libraries import FIELDS, records_of

SEED = 2610
D = 96                                                            # draws per library; no library's was lowered
NAMES = tuple(rl.LIBRARIES)                                       # the index of a library is its place in abi.LIBRARIES
METHODS = {"fold": "fold_mag_f32", "peaks": "find_peaks", "rank": "order_stats", "hist": "level_hist", "bands": "band_power",
           "mask": "mask_test", "harm": "harmonics", "signals": "find_signals", "cfar": "cfar"}
HAS_FIELD = ("peaks", "rank", "bands", "mask", "harm", "signals", "cfar")
# the ownership sizes of each kernel, from the header comment of csrc/x_f32.hip (fold_mag_f32.hip) and csrc/sa_x.hpp
SIZES = {"fold": (4, 1024), "peaks": (2, 4, 128, 256, 512, 1024), "rank": (2, 4, 128, 256, 512, 1024), "hist": (4, 256),
         "bands": (4, 256, 1024), "mask": (4, 64, 256, 1024), "harm": (4, 256, 1024), "signals": (4, 64, 256, 1024),
         "cfar": (4, 128, 1024, 2048)}
FAMILIES = "abcdefg"

Draw = collections.namedtuple("Draw", "index pts field kw")


# ------------------------------------------------------------------------------------------------------------- the rows
def _row(rng, family):
    if family == "a":
        return np.exp(rng.uniform(-20.0, 20.0, N)).astype(np.float32)
    if family == "b":
        r = np.abs(rng.standard_normal(N)).astype(np.float32)
        for _ in range(int(rng.integers(1, 6))):
            r[int(rng.integers(N))] = np.float32(rng.uniform(20.0, 2000.0))
        return r
    if family == "c":
        return rng.integers(0, 4, N).astype(np.float32)
    if family == "d":
        r = np.zeros(N, np.float32)
        n = int(rng.integers(1, 201))
        r[rng.integers(0, N, n)] = np.exp(rng.uniform(-2.0, 8.0, n)).astype(np.float32)
        return r
    if family == "f":
        return np.full(N, (0.0, 1.0, 3.5)[int(rng.integers(3))], np.float32)
    r = np.exp(rng.uniform(-3.0, 3.0, N)).astype(np.float32)
    if family == "g":
        r[int(rng.integers(N))] = np.nan
        return r
    assert family == "e"
    at = np.nonzero(rng.random(N) < 0.002)[0]
    kind = rng.integers(0, 4, at.size)
    r[at[kind == 0]] = np.inf
    r[at[kind == 1]] = -0.0
    r[at[kind == 2]] = np.float32(1e-42)
    r[at[kind == 3]] *= np.float32(-1.0)
    return r


def _rows(rng, R):
    return np.stack([_row(rng, FAMILIES[int(rng.integers(len(FAMILIES)))]) for _ in range(R)])


def _finite(pts):
    """the magnitudes of the finite points, sorted; [1.0] where there is none"""
    a = np.abs(pts[np.isfinite(pts)])
    return np.sort(a) if a.size else np.ones(1, np.float32)


def _f32(v):
    return float(np.float32(v))


# -------------------------------------------------------------------------------------------------------- the integers
def _int(rng, lo, hi, sizes=(), log=False):
    """An int of lo..hi, both included: 20 % an end, 30 % at or one off a multiple of one of ``sizes``, else uniform (``log``:
    uniform in the logarithm)."""
    lo, hi = int(lo), int(hi)
    assert lo <= hi, (lo, hi)
    u = rng.random()
    if u < 0.2:
        return lo if rng.random() < 0.5 else hi
    if u < 0.5 and sizes:
        s = int(sizes[int(rng.integers(len(sizes)))])
        first, last = -(-max(lo - 1, 0) // s), (hi + 1) // s
        if last >= first:
            return min(max(s * int(rng.integers(first, last + 1)) + int(rng.integers(-1, 2)), lo), hi)
    if log:
        return min(max(int(round(float(np.exp(rng.uniform(np.log(max(lo, 1)), np.log(max(hi, 1))))))), lo), hi)
    return int(rng.integers(lo, hi + 1))


def _range(rng, sizes, need=1, bottom=0, top=N):
    """(lo, hi) with bottom <= lo, lo + need <= hi <= top; 15 % at most 300 bins wider than ``need``"""
    lo = _int(rng, bottom, top - need, sizes)
    if rng.random() < 0.15:
        return lo, min(top, lo + need + int(rng.integers(0, 301)))
    return lo, _int(rng, lo + need, top, sizes)


def _field(rng):
    return FIELDS[int(rng.integers(len(FIELDS)))]


# ---------------------------------------------------------------------------------------------------------- the draws
def _draw_fold(rng):
    group = (1, 2, 4, 8)[int(rng.integers(4))]
    pts = _rows(rng, group * int(rng.integers(1, 8 // group + 1)))
    buckets = (1, 2, 4, 8, 16, 32, 64)
    bucket = buckets[int(rng.integers(group == 1, len(buckets)))]     # not both 1
    return pts, None, dict(group=group, bucket=bucket)


def _draw_peaks(rng):
    pts = _rows(rng, int(rng.integers(1, 9)))
    lo, hi = _range(rng, SIZES["peaks"])
    u, a = rng.random(), _finite(pts)
    if u < 0.35:
        threshold = 0.0
    elif u < 0.65:
        threshold = _f32(a[int(rng.integers(a.size))])              # the key of a point: equality decides
    elif u < 0.80:
        threshold = _f32(min(2.0 * float(a[-1]) + 1.0, 3e38))       # above every finite point
    else:
        threshold = _f32(np.exp(rng.uniform(-5.0, 8.0)))
    return pts, _field(rng), dict(k=_int(rng, 1, 32), threshold=threshold, lo=lo, hi=hi,
                                  min_sep=_int(rng, 1, N, SIZES["peaks"], log=True))


def _draw_rank(rng):
    pts = _rows(rng, int(rng.integers(1, 9)))
    lo, hi = _range(rng, SIZES["rank"])
    ranks = [_int(rng, 0, hi - lo - 1, SIZES["rank"]) for _ in range(_int(rng, 1, 8))]
    return pts, _field(rng), dict(ranks=ranks, lo=lo, hi=hi)


def _draw_hist(rng):
    long_group = rng.random() < 0.08
    bucket = (1, 2, 4, 8, 16, 32, 64)[int(rng.integers(7))]
    cols, sizes = N // bucket, tuple(s // bucket for s in SIZES["hist"] if s >= bucket)
    if long_group:                                                 # one group of 64..130 rows over at most 1024 bins: sliced
        R = int(rng.integers(64, 131))
        group = R if rng.random() < 0.5 else None
        lo = _int(rng, 0, cols - 1, sizes)
        hi = min(cols, lo + 1 + int(rng.integers(0, 1024 // bucket)))
    else:
        R = int(rng.integers(1, 9))
        divisors = [g for g in range(1, R + 1) if R % g == 0]
        group = None if rng.random() < 0.15 else divisors[int(rng.integers(len(divisors)))]
        lo, hi = _range(rng, sizes, top=cols)
    pts = _rows(rng, R)
    steps = int(rng.integers(1, 7))                                # the depth of the edge tree, then the levels it serves
    levels = 2 if steps == 1 else _int(rng, (1 << (steps - 1)) + 1, 1 << steps)
    n = levels - 1
    e = np.exp(rng.uniform(-6.0, 6.0, n)).astype(np.float32)
    taken = np.abs(pts[rng.integers(0, R, n), rng.integers(0, N, n)])   # the values of points: a point exactly on an edge
    taken[np.isnan(taken)] = 1.0
    e = np.where(rng.random(n) < 0.3, taken, e)
    e = np.sort(e.view(np.uint32)).view(np.float32)
    for j in range(1, n):
        if rng.random() < 0.15:
            e[j] = e[j - 1]                                        # equal edges: the level between them is empty
    e = np.sort(e.view(np.uint32)).view(np.float32)
    if rng.random() < 0.1:
        e[0] = 0.0
    if rng.random() < 0.1:
        e[-1] = np.inf
    return pts, None, dict(edges=[float(v) for v in e], group=group, bucket=bucket, lo=lo * bucket, hi=hi * bucket)


def _draw_bands(rng):
    from fpga_real_time_fft_analyzer_amd import frames
    pts = _rows(rng, int(rng.integers(1, 9)))
    bands = [_range(rng, SIZES["bands"]) for _ in range(_int(rng, 1, 16))]
    fracs = [(0.0, frames.BANDS_FRAC_MAX, 0.5, float(rng.random()), float(rng.random()))[int(rng.integers(5))]
             for _ in range(_int(rng, 0, 4))]
    return pts, _field(rng), dict(bands=bands, fracs=fracs)


def _limit(rng, pts, up):
    """A limit line of the mask test, float32 [N], relative to the rows it is held against: clear of all finite points, through
    them, or one row's own values; up to three spans of it are gaps (0, a negative value, +inf, a NaN)."""
    a = _finite(pts)
    pos = a[a > 0]
    u = rng.random()
    with np.errstate(over="ignore"):
        if u < 0.35:
            level = 2.0 * float(a[-1]) + 1.0 if up else 0.5 * float(pos[0] if pos.size else 1.0)
            line = level * rng.uniform(1.0, 1.5, N) if up else level * rng.uniform(0.5, 1.0, N)
        elif u < 0.75:
            q = rng.uniform(0.9, 0.9999) if up else rng.uniform(0.0001, 0.1)
            line = float(a[int(q * (a.size - 1))]) * rng.uniform(0.8, 1.25, N)
        else:
            line = np.abs(pts[int(rng.integers(pts.shape[0]))]).astype(np.float64)
        line = np.asarray(line, np.float64).astype(np.float32)
    for _ in range(int(rng.integers(0, 4))):
        at = int(rng.integers(N))
        line[at:at + int(rng.integers(1, 2001))] = (0.0, -1.0, np.inf, np.nan)[int(rng.integers(4))]
    return line


def _draw_mask(rng):
    pts = _rows(rng, int(rng.integers(1, 9)))
    which = int(rng.integers(3))                                   # upper only, lower only, both
    lo, hi = _range(rng, SIZES["mask"])
    return pts, _field(rng), dict(upper=_limit(rng, pts, True) if which != 1 else None,
                                  lower=_limit(rng, pts, False) if which != 0 else None, lo=lo, hi=hi)


def _draw_harm(rng):
    pts = _rows(rng, int(rng.integers(1, 9)))
    sizes = SIZES["harm"]
    order, span = _int(rng, 1, 10), _int(rng, 0, 64, (4, 64))
    top = 8193 if rng.random() < 0.5 else _int(rng, 1, 8193, sizes)
    dc = None if rng.random() < 0.4 else _int(rng, 0, min(top - 1, 130) if rng.random() < 0.5 else top - 1, sizes)
    if dc is None and span + 1 >= top:
        dc = _int(rng, 0, top - 1, sizes)
    first = span + 1 if dc is None else dc
    lo = None if rng.random() < 0.4 else _int(rng, first, top - 1, sizes)
    hi = None if rng.random() < 0.4 else _int(rng, (first if lo is None else lo) + 1, top, sizes)
    u = rng.random()
    fund = None if u < 0.4 else -1 if u < 0.5 else _int(rng, first, top - 1, sizes)
    return pts, _field(rng), dict(order=order, span=span, lo=lo, hi=hi, fund=fund, dc=dc, top=top)


def _draw_signals(rng):
    R = int(rng.integers(1, 9))
    pts = _rows(rng, R)
    sizes = SIZES["signals"]
    lo, hi = _range(rng, sizes)

    def level(row):
        a = _finite(row)
        return a[int((0.5, 0.9, 0.99, 0.999)[int(rng.integers(4))] * (a.size - 1))]

    if rng.random() < 0.7:
        u = rng.random()
        threshold = 0.0 if u < 0.1 else _f32(level(pts)) if u < 0.7 else float("inf") if u < 0.75 else _f32(np.exp(rng.uniform(-3.0, 6.0)))
    else:                                                          # one per row, keyed like a point: 0, +inf, a NaN, a negative value
        threshold = np.zeros(R, np.float32)
        for r in range(R):
            u = rng.random()
            threshold[r] = level(pts[r]) if u < 0.6 else 0.0 if u < 0.7 else np.inf if u < 0.8 else np.nan if u < 0.9 else -level(pts[r])
    gap = 0 if rng.random() < 0.35 else _int(rng, 0, N - 1, sizes, log=True)
    min_width = 1 if rng.random() < 0.4 else _int(rng, 1, N, sizes, log=True)
    return pts, _field(rng), dict(k=_int(rng, 1, 32), threshold=threshold, lo=lo, hi=hi, gap=gap, min_width=min_width)


def _draw_cfar(rng):
    pts = _rows(rng, int(rng.integers(1, 9)))
    sizes = SIZES["cfar"]
    train = (1, 2, 4, 8, 16, 32, 64)[int(rng.integers(7))]
    guard = _int(rng, 0, 64, (4, 64))
    need, u = 2 * guard + 2, rng.random()
    if u < 0.15:                                                   # ends inside the first tile
        lo = _int(rng, 0, 2047 - need, sizes)
        hi = _int(rng, lo + need, 2047, sizes)
    elif u < 0.30:                                                 # ends inside the last tile
        hi = _int(rng, 14337, N - 1, sizes)
        lo = _int(rng, 0, hi - need, sizes)
    else:
        lo, hi = _range(rng, sizes, need=need)
    return pts, _field(rng), dict(train=train, guard=guard, mode=("ca", "go", "so")[int(rng.integers(3))],
                                  what=("ratio", "floor")[int(rng.integers(2))], lo=lo, hi=hi)


_DRAW = {"fold": _draw_fold, "peaks": _draw_peaks, "rank": _draw_rank, "hist": _draw_hist, "bands": _draw_bands, "mask": _draw_mask,
         "harm": _draw_harm, "signals": _draw_signals, "cfar": _draw_cfar}


def make_draws(name, seed=SEED, count=D):
    """The draws of a library, made anew: a tuple of ``count`` Draws whose arrays are read-only."""
    rng = np.random.default_rng([seed, NAMES.index(name)])
    out = []
    for i in range(count):
        pts, field, kw = _DRAW[name](rng)
        for a in (pts, *(v for v in kw.values() if isinstance(v, np.ndarray))):
            a.setflags(write=False)
        out.append(Draw(i, pts, field, kw))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def draws(name):
    """The D draws of a library at SEED, made once and shared by every test."""
    return make_draws(name)


def show(name, draw):
    """One line that says which draw it is and is enough to repeat it: the library, the index and the full arguments, an
    array by its values where it is short and by where it comes from where it is a line of 16384 limits."""
    def text(key, v):
        if isinstance(v, np.ndarray):
            return repr(v.tolist()) if v.size <= 8 else f"drawn_cases.draws({name!r})[{draw.index}].kw[{key!r}]"
        return repr(v)
    kw = ", ".join(f"{key}={text(key, v)}" for key, v in draw.kw.items())
    return (f"library {name}, draw {draw.index}: SpectrumChain.{METHODS[name]}(records_of(drawn_cases.draws({name!r})[{draw.index}].pts, "
            f"{draw.field!r}){', field=' + repr(draw.field) if name in HAS_FIELD else ''}, {kw})  [R = {draw.pts.shape[0]}, SEED = {SEED}]")


# ------------------------------------------------------------------------------------------- the rules and the mirrors
def accept(name, field, kw):
    """The rule function ``frames._x_args`` of the library on the arguments of a draw: it raises ValueError or returns."""
    from fpga_real_time_fft_analyzer_amd import frames
    k = kw
    if name == "fold":
        return frames._fold_args(k["group"], k["bucket"])
    if name == "peaks":
        return frames._peaks_args(k["k"], k["threshold"], k["lo"], k["hi"], k["min_sep"], field)
    if name == "rank":
        return frames._rank_args(k["ranks"], k["lo"], k["hi"], field)
    if name == "hist":
        return frames._hist_args(k["edges"], k["group"], k["bucket"], k["lo"], k["hi"])
    if name == "bands":
        return frames._bands_args(k["bands"], k["fracs"], field)
    if name == "mask":
        return frames._mask_args(k["upper"], k["lower"], k["lo"], k["hi"], field)
    if name == "harm":
        return frames._harm_args(k["order"], k["span"], k["lo"], k["hi"], k["fund"], k["dc"], k["top"], field)
    if name == "signals":
        if not isinstance(k["threshold"], np.ndarray):
            frames._threshold_key(k["threshold"])
        return frames._signals_args(k["k"], k["lo"], k["hi"], k["gap"], k["min_width"], field)
    assert name == "cfar", name
    return frames._cfar_args(k["train"], k["guard"], k["mode"], k["what"], k["lo"], k["hi"], field)


def mirror(name, pts, field, kw):
    """The result of the library's numpy mirror as a tuple of arrays, one per output of the call: fold (peak, power), peaks
    (mag, bin, count), rank (values,), hist (counters,), bands (power, cross), mask (records, summary), harm (records,),
    signals (records, stats), cfar (values,)."""
    from fpga_real_time_fft_analyzer_amd import frames
    if name == "fold":
        return frames.fold_of_mags(pts, **kw)[:2]
    if name == "peaks":
        return frames.peaks_of_rows(pts, **kw)
    if name == "hist":
        return (frames.hist_of_rows(pts, **kw),)
    fn = {"rank": frames.ranks_of_rows, "bands": frames.bands_of_rows, "mask": frames.mask_of_rows, "harm": frames.harm_of_rows,
          "signals": frames.signals_of_rows, "cfar": frames.cfar_of_rows}[name]
    out = fn(records_of(pts, field), field=field, **kw)
    return out if isinstance(out, tuple) else (out,)


@functools.lru_cache(maxsize=None)
def wanted(name):
    """The mirror's result of every draw of a library, computed once and shared."""
    return tuple(mirror(name, d.pts, d.field, d.kw) for d in draws(name))


# ------------------------------------------------------------------------------------------------- the call's outputs
def outputs(name, R, kw):
    """The tensors a call writes through ``out=`` arguments: (argument, shape, numpy dtype) each."""
    from fpga_real_time_fft_analyzer_amd import frames
    if name == "fold":
        return [("out", (R // kw["group"], N // kw["bucket"], 2), "float32")]
    if name == "peaks":
        return [("out", (R, kw["k"], 2), "int32")]                    # count is allocated by the call
    if name == "rank":
        return [("out", (R, len(kw["ranks"])), "float32")]
    if name == "hist":
        return [("out", (R // (kw["group"] or R), (kw["hi"] - kw["lo"]) // kw["bucket"], len(kw["edges"]) + 1), "uint32")]
    if name == "bands":
        nb, nq = len(kw["bands"]), len(kw["fracs"])
        return [("power", (R, nb), "float64")] + ([("cross", (R, nb, nq), "int32")] if nq else [])
    if name == "mask":
        return [("out", (R, frames.MASK_ROW.itemsize // 4), "int32"), ("summary", (4,), "int32")]
    if name == "harm":
        return [("out", (R, frames.HARM_ROW.itemsize // 4), "int32")]
    if name == "signals":
        return [("out", (R, kw["k"], frames.SIGNAL.itemsize // 4), "int32"), ("stats", (R, 3), "int32")]
    assert name == "cfar", name
    return [("out", (R, N), "float32")]


# what a method allocates itself and only returns, one element per row: library -> (name, place in the returned tuple, dtype)
RETURNED = {"peaks": (("count", 2, "int32"),)}


def result(name, arrays, returned, kw):
    """What the device wrote, in the form of mirror(): ``arrays`` is argument -> the host copy of that output tensor, in the
    dtype and shape of outputs(); ``returned`` the host copies of what the method returned (peaks: its count is the third)."""
    from fpga_real_time_fft_analyzer_amd import frames
    if name == "fold":
        return arrays["out"][..., 0], arrays["out"][..., 1]
    if name == "peaks":
        return arrays["out"][..., 0].view(np.float32), arrays["out"][..., 1], returned[2]
    if name == "bands":
        power = arrays["power"]
        return power, arrays["cross"] if "cross" in arrays else np.zeros(power.shape + (0,), np.int32)
    if name == "mask":
        return arrays["out"].view(frames.MASK_ROW)[:, 0], arrays["summary"]
    if name == "harm":
        return (arrays["out"].view(frames.HARM_ROW)[:, 0],)
    if name == "signals":
        return arrays["out"].view(frames.SIGNAL)[..., 0], arrays["stats"]
    return (arrays["out"],)


# ------------------------------------------------------------------------------------------------------- the comparer
def _same_words(a, b):
    """None where two arrays of 4-byte elements are equal bit for bit, else where they differ"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype} {a.shape} against {b.dtype} {b.shape}"
    x, y = a.view(np.uint32), b.view(np.uint32)
    if np.array_equal(x, y):
        return None
    at = np.argwhere(x != y)
    return f"{len(at)} words differ, the first at {at[0].tolist()}: {int(x[tuple(at[0])]):#x} against {int(y[tuple(at[0])]):#x}"


def _same_but_nans(a, b):
    """_same_words for float32 values of which a NaN is compared by position: the header gives its payload no meaning"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype} {a.shape} against {b.dtype} {b.shape}"
    nan = np.isnan(b)
    if not np.array_equal(np.isnan(a), nan):
        return f"NaNs at other places, the first at {np.argwhere(np.isnan(a) != nan)[0].tolist()}"
    return _same_words(np.where(nan, np.float32(0.0), a), np.where(nan, np.float32(0.0), b))


def compare(name, got, want):
    """None where the result ``got`` equals the mirror's ``want`` -- both in the form of mirror() -- else what differs.  Bits on
    integer views, every array of the call; a NaN by position where the library's own test file compares it so: the float32
    power of the fold, the float64 sums of bands, harm and signals, the floats of a mask record."""
    from test_f32_bands_cpu import same_bits
    from test_f32_harm_cpu import same_records as same_harm
    from test_f32_mask_cpu import same_records as same_mask
    from test_f32_signals_cpu import same_result
    if len(got) != len(want):
        return f"{len(got)} arrays against {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"array {i}: {g.dtype} {g.shape} against {w.dtype} {w.shape}"
    if name in ("fold", "peaks"):
        same = (_same_words, _same_but_nans) if name == "fold" else (_same_words,) * 3
        for label, fn, g, w in zip(("peak", "power") if name == "fold" else ("mag", "bin", "count"), same, got, want):
            bad = fn(g, w)
            if bad:
                return f"{label}: {bad}"
        return None
    if name in ("rank", "cfar", "hist"):
        return _same_words(got[0], want[0])
    if name == "bands":
        if not same_bits(got[0], want[0]):
            return f"power: {np.argwhere(~((got[0] == want[0]) | (np.isnan(got[0]) & np.isnan(want[0]))))[:5].tolist()}"
        bad = _same_words(got[1], want[1])
        return f"cross: {bad}" if bad else None
    if name == "mask":
        if got[0].dtype != want[0].dtype or not same_mask(got[0], want[0]):
            rows = [r for r in range(min(len(got[0]), len(want[0]))) if not same_mask(got[0][r:r + 1], want[0][r:r + 1])]
            return f"records: rows {rows[:5]}: {got[0][rows[:2]].tolist()} against {want[0][rows[:2]].tolist()}"
        bad = _same_words(got[1], want[1])
        return f"summary: {bad}: {got[1].tolist()} against {want[1].tolist()}" if bad else None
    if name == "harm":
        return same_harm(got[0], want[0])
    assert name == "signals", name
    return same_result(got, want)


def plain_arrays(result_):
    """(label, array) of every plain array of a result in the form of mirror(): an array itself, or each field of a
    structured one, as a view that writes through."""
    out = []
    for i, a in enumerate(result_):
        if a.dtype.names:
            out += [(f"{i}.{f}", a[f]) for f in a.dtype.names]
        else:
            out.append((str(i), a))
    return out


# ----------------------------------------------------------------------------------------------- what a draw launches
def hist_slices(rows, group, bucket, lo=0, hi=N):
    """The row slices of a group, as sa_hist_f32 (csrc/hist_f32.hip) decides them from kHistOwnersFew = 256, kHistOwnersAim =
    512 and kHistSliceRowsMin = 32 of csrc/sa_hist.hpp: G x tiles workgroups own their counters; below 256 of them a group
    of 64 rows or more is cut so that about 512 workgroups run."""
    tile = 256
    tiles = (hi - 1) // tile - lo // tile + 1
    owners = rows // group * tiles
    if owners >= 256:
        return 1
    s = min(-(-512 // owners), group // 32)
    return s if s >= 2 else 1


def kernels(name, R, field, kw):
    """The kernel instantiations a draw launches, as kernel_inventory.key_of keys them."""
    code = FIELDS.index(field)
    if name == "fold":
        return (f"fold_mag_f32_kernel<{kw['bucket'].bit_length() - 1}>",)
    if name == "hist":
        levels, steps = len(kw["edges"]) + 1, 1
        while (1 << steps) < levels:
            steps += 1
        sliced = hist_slices(R, kw["group"] or R, kw["bucket"], kw["lo"], kw["hi"]) > 1
        return (("hist_zero_kernel",) if sliced else ()) + (f"hist_f32_kernel<{steps}>",)
    if name == "bands":
        return (f"bands_f32_kernel<{code}, {'true' if len(kw['fracs']) > 0 else 'false'}>",)
    if name == "mask":
        up, low = ("true" if kw[k] is not None else "false" for k in ("upper", "lower"))
        return (f"mask_f32_kernel<{code}, {up}, {low}>", "mask_summary_kernel")       # the draws ask for the summary
    return (f"{name}_f32_kernel<{code}>",)


# ------------------------------------------------------------------------------------------- what the draws must reach
KINDS = {
    "fold": tuple(f"bucket {w}" for w in (1, 2, 4, 8, 16, 32, 64)) + ("group 1", "group above 1"),
    "peaks": ("a row with no candidate", "a count above k", "a count below k", "two candidates closer than min_sep"),
    "rank": ("rank 0", "rank hi - lo - 1", "ties at the rank"),
    "hist": ("an empty level", "a point exactly on an edge", "the sliced form"),
    "bands": ("a crossing reached", "a crossing of -1", "nb = 1", "nb = 16", "nq = 0"),
    "mask": tuple(f"{limits}: a row that {what}" for limits in ("upper only", "lower only", "both") for what in ("violates", "passes")),
    "harm": ("a fixed fundamental", "a searched fundamental", "a harmonic that folds", "order = 1", "order = 10"),
    "signals": ("a row with no segment", "more segments than k", "a bridged gap", "a segment dropped by min_width"),
    "cfar": tuple(f"{m} {w}" for m in ("ca", "go", "so") for w in ("ratio", "floor"))
            + ("an inf in the result", "a NaN in the result", "ends inside the first tile", "ends inside the last tile"),
}


def kinds(name, draw, want):
    """The kinds of KINDS[name] that a draw reaches, read from its arguments and the mirror's result ``want``."""
    from fpga_real_time_fft_analyzer_amd import frames
    kw, pts, out = draw.kw, draw.pts, set()
    R = pts.shape[0]

    def add(kind, reached):
        assert kind in KINDS[name], kind
        if reached:
            out.add(kind)

    if name == "fold":
        add(f"bucket {kw['bucket']}", True)
        add("group 1" if kw["group"] == 1 else "group above 1", True)
    elif name == "peaks":
        mag, bins, count = want
        add("a row with no candidate", (count == 0).any())
        add("a count above k", (count > kw["k"]).any())
        add("a count below k", ((count > 0) & (count < kw["k"])).any())
        _, every, _ = frames.peaks_of_rows(pts, k=32, threshold=kw["threshold"], lo=kw["lo"], hi=kw["hi"], min_sep=1)
        near = False                                               # among the 32 strongest candidates of a row
        for r in range(R):
            b = np.sort(every[r][every[r] >= 0])
            near |= b.size >= 2 and int(np.diff(b).min()) < kw["min_sep"]
        add("two candidates closer than min_sep", near)
    elif name == "rank":
        m = kw["hi"] - kw["lo"]
        add("rank 0", 0 in kw["ranks"])
        add("rank hi - lo - 1", m - 1 in kw["ranks"])
        s = np.sort(frames._key(np.ascontiguousarray(pts))[:, kw["lo"]:kw["hi"]], axis=1)
        add("ties at the rank", any((r > 0 and (s[:, r] == s[:, r - 1]).any()) or (r < m - 1 and (s[:, r] == s[:, r + 1]).any())
                                    for r in kw["ranks"]))
    elif name == "hist":
        keys = frames._hist_edge_keys(kw["edges"])
        equal = np.nonzero(keys[1:] == keys[:-1])[0]
        add("an empty level", equal.size > 0 and not want[0][..., equal + 1].any())
        add("a point exactly on an edge", np.isin(frames._key(np.ascontiguousarray(pts))[:, kw["lo"]:kw["hi"]], keys).any())
        add("the sliced form", "hist_zero_kernel" in kernels(name, R, draw.field, kw))
    elif name == "bands":
        add("a crossing reached", (want[1] >= 0).any())
        add("a crossing of -1", (want[1] == -1).any())
        add("nb = 1", len(kw["bands"]) == 1)
        add("nb = 16", len(kw["bands"]) == 16)
        add("nq = 0", len(kw["fracs"]) == 0)
    elif name == "mask":
        limits = "both" if kw["upper"] is not None and kw["lower"] is not None else "upper only" if kw["upper"] is not None else "lower only"
        failed = (want[0]["over"] > 0) | (want[0]["under"] > 0)
        add(f"{limits}: a row that violates", failed.any())
        add(f"{limits}: a row that passes", (~failed).any())
    elif name == "harm":
        searched = kw["fund"] in (None, -1)
        add("a searched fundamental" if searched else "a fixed fundamental", True)
        k1 = want[0]["bin"][:, 0].astype(np.int64)
        h = np.arange(2, kw["order"] + 1)
        add("a harmonic that folds", ((k1[:, None] * h) % N > N // 2).any())
        add("order = 1", kw["order"] == 1)
        add("order = 10", kw["order"] == 10)
    elif name == "signals":
        stats = want[1]
        add("a row with no segment", (stats[:, 0] == 0).any())
        add("more segments than k", (stats[:, 0] > kw["k"]).any())
        x = records_of(pts, draw.field)
        wide = dict(kw, k=1, min_width=1)
        runs = frames.signals_of_rows(x, field=draw.field, **wide)[1][:, 0]
        add("a bridged gap", (frames.signals_of_rows(x, field=draw.field, **dict(wide, gap=0))[1][:, 0] > runs).any())
        add("a segment dropped by min_width", (runs > stats[:, 0]).any())
    else:
        assert name == "cfar", name
        add(f"{kw['mode']} {kw['what']}", True)
        add("an inf in the result", np.isinf(want[0]).any())
        add("a NaN in the result", np.isnan(want[0]).any())
        add("ends inside the first tile", 0 < kw["hi"] < 2048)
        add("ends inside the last tile", N - 2048 < kw["hi"] < N)
    return out
