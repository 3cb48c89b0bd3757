"""CPU: the argument rules of the nine handle-less reductions, stated once in frames.py (``frames._x_args``) and reached by the
device's wrappers through ``reductions._rules``: a numpy mirror and its wrapper accept the same arguments and refuse the
rest with the same text, the wrapper with the code SA_EINVAL.

For each reduction a grid of argument tuples is drawn and both sides are called on every tuple: the mirror's rule function
and the wrapper's class-level ``_x_args`` on ``object.__new__(SpectrumChain)``.  No device, no library: a rule function
looks at its arguments only.  An axis of a grid lists the values of one argument, the first of them good: the ends of its
range and one step outside, ``True``, ``2.0``, a str and None where an int belongs, a NaN, a negative value and a str where
a threshold belongs.  The grid is the product of the axes where that has at most ``FULL`` tuples.  A longer product is cut
down to what decides an order of rules, which of two faults wins: every pair of arguments takes all its pairs of values
with the others at their first value, and all of that is crossed with every value of ``field``, so that a bad field
stands beside every other fault alone and beside every pair of them.

``TEXTS`` lists, per reduction, the texts its rule function can raise on its grid: the grid must draw every one at least once
and accept at least one tuple, so that the test cannot pass by drawing nothing.  ``NAMED`` are the calls in which the two
statements of the rules differed while each file had its own.
"""
import itertools

import numpy as np
import pytest

from conftest import N

FULL = 1 << 16
NAN, INF = float("nan"), float("inf")
LIM = object()                                          # a limit of the mask test: counted, never looked at
FIELD = (None, "peak", "power", "mag", 0)
NO_FIELD = "field must be None, 'peak' or 'power'"
RANGE = "the range must be 0 <= lo < hi <= 16384"
THRESHOLDS = (0.0, INF, 1, np.float32(0.5), NAN, -1.0, -0.0, "1", True, None)
NO_THRESHOLD = ("threshold must be a number", "threshold must be +0.0 .. +inf: no NaN, no sign bit")
LO = (0, N - 1, -1, True, 2.0, "0", None)
HI = (N, 1, N + 1, True, 2.0, "5", None)


def no_int(*names):
    return tuple(f"{name} must be an int" for name in names)


# reduction -> (the arguments in the order of both rule functions, one axis each)
AXES = {
    "fold": dict(group=(2, 1, 128, 0, 3, 256, True, 2.0, "2", None), bucket=(2, 1, 64, 0, 3, 128, True, 2.0, "2", None)),
    "peaks": dict(k=(8, 1, 32, 0, 33, True, 2.0, "8", None), threshold=THRESHOLDS, lo=LO, hi=HI,
                  min_sep=(1, N, 0, N + 1, True, 2.0, "1", None), field=FIELD),
    "rank": dict(ranks=([0], (0,) * 8, np.array([0]), [N - 1], [], [0] * 9, "12", 5, None, [True], [1.0], ["1"], [None], [-1], [N]),
                 lo=LO, hi=HI, field=FIELD),
    "hist": dict(edges=([1.0], [0.0, INF], list(range(63)), [], list(range(64)), "12", None, [True], ["1"], [NAN], [-1.0],
                        [2.0, 1.0]),
                 group=(None, 1, 1 << 24, 0, (1 << 24) + 1, True, 2.0, "2"), bucket=(1, 64, 0, 3, 128, True, 2.0, "2", None),
                 lo=(0, 64, 128, -1, 8, True, 2.0, "0", None), hi=(N, 128, N + 1, N - 8, True, 2.0, "5", None)),
    "bands": dict(bands=([(0, N)], [(0, 1)] * 16, [np.array([5, 6])], [], [(0, 1)] * 17, "ab", 5, None, [5], ["ab"], [(0, 1, 2)],
                         [(True, 5)], [(0.0, 5)], [("0", 5)], [(None, 5)], [(5, 5)], [(-1, 5)], [(0, N + 1)]),
                  fracs=((), (0.5,), (0.0, 1.0 - 2.0 ** -32), [0.5] * 4, (0.5,) * 5, 0.5, "12", None, (True,), ("1",), (NAN,),
                         (-0.1,), (1.0,)),
                  field=FIELD),
    "mask": dict(upper=(LIM, None), lower=(None, LIM), lo=LO, hi=HI, field=FIELD),
    "harm": dict(order=(5, 1, 10, 0, 11, True, 2.0, "5", None), span=(3, 0, 64, -1, 65, True, 2.0, "3", None),
                 lo=(None, 4, 8192, 3, 8193, True, 2.0, "4"), hi=(None, 8193, 5, 4, 8194, True, 2.0, "5"),
                 fund=(None, -1, 4, 8192, 3, 8193, True, 2.0, "4"), dc=(None, 0, 8192, -1, 8193, True, 2.0, "0"),
                 top=(8193, 5, 4, 0, 8194, True, 2.0, "5", None), field=FIELD),
    "signals": dict(k=(16, 1, 32, 0, 33, True, 2.0, "8", None), threshold=THRESHOLDS, lo=LO, hi=HI,
                    gap=(0, N - 1, -1, N, True, 2.0, "0", None), min_width=(1, N, 0, N + 1, True, 2.0, "1", None), field=FIELD),
    "cfar": dict(train=(16, 1, 64, 0, 3, 128, True, 2.0, "4", None), guard=(2, 0, 64, -1, 65, True, 2.0, "2", None),
                 mode=("ca", "go", "so", "os", 0, None), what=("ratio", "floor", "db", 1, None),
                 lo=(0, 10, N - 6, -1, True, 2.0, "0", None), hi=(N, 16, 15, 130, 129, N + 1, True, 2.0, "5", None), field=FIELD),
}
# reduction -> every text its rule function raises on the grid above
TEXTS = {
    "fold": ("group must be one of (1, 2, 4, 8, 16, 32, 64, 128)", "bucket must be one of (1, 2, 4, 8, 16, 32, 64)",
             "group = bucket = 1 folds nothing"),
    "peaks": no_int("k", "lo", "hi", "min_sep") + ("k must be 1..32",) + NO_THRESHOLD + (RANGE, "min_sep must be 1..16384", NO_FIELD),
    "rank": no_int("lo", "hi") + (RANGE, "ranks must be a sequence of 1..8 ints", "a rank must be an int in 0..16383",
                                  "a rank must be an int in 0..0", NO_FIELD),
    "hist": no_int("bucket", "lo", "hi", "group") + (
        "group must be 1..16777216", "bucket must be one of (1, 2, 4, 8, 16, 32, 64)", "edges must be a sequence of 1..63 numbers",
        "an edge must be a number", "an edge must be +0.0 .. +inf: no NaN, no sign bit", "the edges must not decrease",
        RANGE + ", both multiples of the bucket"),
    "bands": ("bands must be a sequence of 1..16 (lo, hi) pairs", "a band must be a (lo, hi) pair", "lo and hi of a band must be ints",
              "a band must be 0 <= lo < hi <= 16384", "fracs must be a sequence of 0..4 numbers",
              "a fraction must be a number in 0 .. 1 - 2^-32", NO_FIELD),
    "mask": no_int("lo", "hi") + (RANGE, NO_FIELD, "upper and lower are both None: no limit at all"),
    "harm": no_int("order", "span", "lo", "hi", "fund", "dc", "top") + (
        "span must be 0..64", "order must be 1..10", "the analysed bins must be 0 <= dc < top <= 8193",
        "the search range must be dc <= lo < hi <= top", "fund must be None, -1 or a bin in [dc, top)", NO_FIELD),
    "signals": no_int("k", "lo", "hi", "gap", "min_width") + ("k must be 1..32", RANGE, "gap must be 0..16383",
                                                               "min_width must be 1..16384", NO_FIELD) + NO_THRESHOLD,
    "cfar": no_int("train", "guard", "lo", "hi") + (
        "train must be one of (1, 2, 4, 8, 16, 32, 64)", "guard must be 0..64", "mode must be 'ca', 'go' or 'so'",
        "what must be 'ratio' or 'floor'", RANGE, "the range must hold 2 * guard + 2 bins or more", NO_FIELD),
}
# (reduction, arguments that differ from the first value of their axes, the refusal of both sides)
NAMED = [
    ("peaks", dict(threshold="1"), "threshold must be a number"),                      # the mirror took both as numbers
    ("peaks", dict(threshold=True), "threshold must be a number"),
    ("peaks", dict(k=0, threshold=NAN, lo=5, hi=5, min_sep=0), "k must be 1..32"),     # the mirror had one text for the six
    ("peaks", dict(threshold=NAN, lo=5, hi=5, min_sep=0), NO_THRESHOLD[1]),
    ("peaks", dict(lo=5, hi=5, min_sep=0, field="mag"), RANGE),
    ("peaks", dict(min_sep=0, field="mag"), "min_sep must be 1..16384"),
    ("hist", dict(group=2.0, bucket=True), "bucket must be an int"),                   # the mirror looked at the group first
    ("hist", dict(group=2.0, hi="5"), "hi must be an int"),
    ("hist", dict(group=2.0), "group must be an int"),
    ("cfar", dict(train=3, field="mag"), "train must be one of (1, 2, 4, 8, 16, 32, 64)"),      # the wrapper looked at the field first
    ("cfar", dict(guard=65, field=0), "guard must be 0..64"),
    ("cfar", dict(mode="os", field="mag"), "mode must be 'ca', 'go' or 'so'"),
    ("cfar", dict(what="db", field="mag"), "what must be 'ratio' or 'floor'"),
    ("cfar", dict(lo=10, hi=15, field="mag"), "the range must hold 2 * guard + 2 bins or more"),
    ("cfar", dict(train=True, field="mag"), "train must be an int"),
    ("cfar", dict(field="mag"), NO_FIELD),
]
WRAPPER = dict(fold="_log2_fold")                       # the other eight are _<reduction>_args


def grid(axes: dict) -> list:
    """The argument tuples of one reduction (module docstring)."""
    values = list(axes.values())
    if np.prod([len(v) for v in values]) <= FULL:
        return list(itertools.product(*values))
    assert list(axes)[-1] == "field"
    first = [v[0] for v in values]
    out = []
    for i, j in itertools.combinations(range(len(values) - 1), 2):
        for a, b, f in itertools.product(values[i], values[j], values[-1]):
            t = list(first)
            t[i], t[j], t[-1] = a, b, f
            out.append(tuple(t))
    return out


def both_sides(name):
    """``(mirror, wrapper)`` of a reduction: each takes the argument tuple and gives the text of its refusal, or None."""
    from fpga_real_time_fft_analyzer_amd import abi, frames
    from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain
    rule = getattr(frames, f"_{name}_args")
    method = getattr(object.__new__(SpectrumChain), WRAPPER.get(name, f"_{name}_args"))

    def mirror(args):
        try:
            if name == "signals":                     # the mirror keys a scalar threshold after the other rules
                k, threshold, *rest = args
                rule(k, *rest)
                frames._threshold_key(threshold)
            else:
                rule(*args)
        except ValueError as e:
            return str(e)

    def wrapper(args):
        try:
            method(*args)
        except abi.SpecanError as e:
            prefix = f"specan error {abi.SA_EINVAL}: "
            assert e.code == abi.SA_EINVAL and str(e).startswith(prefix), (name, args)
            return str(e)[len(prefix):]

    return mirror, wrapper


@pytest.mark.parametrize("name", list(AXES))
def test_mirror_and_wrapper_refuse_alike(name):
    mirror, wrapper = both_sides(name)
    tuples = grid(AXES[name])
    assert len(set(map(repr, tuples))) >= 100 and tuples[0] == tuple(v[0] for v in AXES[name].values())
    drawn = set()
    for args in tuples:
        m, w = mirror(args), wrapper(args)
        assert m == w, (name, args)
        drawn.add(m)
    assert None in drawn and mirror(tuples[0]) is None, name       # the first value of every axis is good
    assert drawn - {None} == set(TEXTS[name]), (name, drawn ^ ({None} | set(TEXTS[name])))


@pytest.mark.parametrize("name, changed, text", NAMED, ids=[f"{name}-{'-'.join(changed)}" for name, changed, _ in NAMED])
def test_where_the_two_statements_differed(name, changed, text):
    mirror, wrapper = both_sides(name)
    assert set(changed) <= set(AXES[name])
    args = tuple(changed.get(arg, values[0]) for arg, values in AXES[name].items())
    assert (mirror(args), wrapper(args)) == (text, text)


def test_the_mirrors_refuse_by_their_rule_functions():
    """What the rule functions refuse, the mirrors refuse in the same words, before they look at the points; the histogram's
    mirror takes ``group=None``, all rows, as ``level_hist`` does."""
    from fpga_real_time_fft_analyzer_amd import frames
    bad = np.zeros((3, 5), np.float64)                  # right for no mirror
    for call, text in ((lambda: frames.fold_of_mags(bad, 1, 1), "group = bucket = 1 folds nothing"),
                       (lambda: frames.peaks_of_rows(bad, threshold="1"), "threshold must be a number"),
                       (lambda: frames.peaks_of_rows(bad, threshold=True), "threshold must be a number"),
                       (lambda: frames.peaks_of_rows(bad, k=0, min_sep=0), "k must be 1..32"),
                       (lambda: frames.peaks_of_rows(bad, lo=5, hi=5, min_sep=0), RANGE),
                       (lambda: frames.ranks_of_rows(bad, [N], field="mag"), "a rank must be an int in 0..16383"),
                       (lambda: frames.hist_of_rows(bad, [1.0], group=2.0, bucket=True), "bucket must be an int"),
                       (lambda: frames.mask_of_rows(bad, None, field="mag"), NO_FIELD),
                       (lambda: frames.mask_of_rows(bad, [1.0] * N), "upper must be None or a float32 [16384] array"),
                       (lambda: frames.cfar_of_rows(bad, train=3, field="mag"), "train must be one of (1, 2, 4, 8, 16, 32, 64)"),
                       (lambda: frames.peaks_of_rows(bad), "points must be float32 [R, 16384]"),
                       (lambda: frames.cfar_of_rows(bad, field="peak"), "points must be float32 [R, 16384, 2]")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    pts = np.zeros((3, N), np.float32)
    assert np.array_equal(frames.hist_of_rows(pts, [1.0], group=None, bucket=64), frames.hist_of_rows(pts, [1.0], group=3, bucket=64))
    assert frames.hist_of_rows(pts[:0], [1.0], group=None, bucket=64).shape == (0, 256, 2)
