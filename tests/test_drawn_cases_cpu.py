"""CPU: the guard of tests/drawn_cases.py, on the numpy mirrors alone.  The GPU tests of tests/test_gpu_f32_drawn.py hold every
drawn call to its mirror; what they are worth depends on the draws, and this file holds the draws to that:

- every draw is accepted by the library's rule function ``frames._x_args`` and by its mirror, and SEED gives the same draws
  twice, one library's not depending on another's;
- the kernel instantiations the draws of a library launch are exactly the instantiations libspecan_x.so holds, so that a kernel
  form added later fails here until a draw reaches it;
- every kind of outcome of drawn_cases.KINDS is reached by LEAST draws or more, counted on the mirror's results;
- the comparer sees one flipped bit in every array of every library's result.

The long parts are one test per library, so that a failure names the library."""
import collections
import copy

import numpy as np
import pytest

import drawn_cases as dc
import kernel_inventory as ki
import reduction_libraries as rl
from conftest import N

LEAST = 3


def _bytes(v):
    return (v.dtype.str, v.shape, v.tobytes()) if isinstance(v, np.ndarray) else v


def _identity(draw):
    """a draw as plain values that compare equal exactly where the draws are the same, NaNs included"""
    return draw.index, _bytes(draw.pts), draw.field, {k: _bytes(v) for k, v in draw.kw.items()}


def reached(name, draws, wants):
    """kind -> the number of draws that reach it"""
    count = collections.Counter({k: 0 for k in dc.KINDS[name]})
    for d, w in zip(draws, wants):
        count.update(dc.kinds(name, d, w))
    return count


def launched(name, draws):
    return {k for d in draws for k in dc.kernels(name, d.pts.shape[0], d.field, d.kw)}


def test_the_table_names_the_nine_libraries():
    assert dc.NAMES == tuple(rl.LIBRARIES) and len(dc.NAMES) == 9 and dc.D == 96
    for table in (dc.METHODS, dc.SIZES, dc.KINDS, dc._DRAW):
        assert set(table) == set(dc.NAMES)
    assert set(dc.HAS_FIELD) == set(dc.NAMES) - {"fold", "hist"}


@pytest.mark.parametrize("name", dc.NAMES)
def test_every_draw_is_accepted_and_the_seed_repeats(name):
    from fpga_real_time_fft_analyzer_amd import frames
    draws = dc.draws(name)
    assert len(draws) == dc.D and [d.index for d in draws] == list(range(dc.D))
    fields = set()
    for d, want in zip(draws, dc.wanted(name)):                    # wanted(): the mirror raised no ValueError
        R = d.pts.shape[0]
        assert d.pts.dtype == np.float32 and d.pts.shape == (R, N) and not d.pts.flags.writeable, dc.show(name, d)
        assert 1 <= R <= 8 or (name == "hist" and 64 <= R <= 130), dc.show(name, d)
        assert d.field in rl.FIELDS and (d.field is None or name in dc.HAS_FIELD)
        dc.accept(name, d.field, d.kw)                               # the rule function raises no ValueError
        assert all(isinstance(a, np.ndarray) for a in want)
        spec = dc.outputs(name, R, d.kw)                           # the bytes the device is given are those of the mirror's arrays
        words = sum(int(np.prod(shape)) * np.dtype(t).itemsize for _, shape, t in spec)
        held = sum(a.nbytes for a in want) - (want[2].nbytes if name == "peaks" else 0)
        assert words == held, (dc.show(name, d), words, held)
        fields.add(d.field)
    assert fields == (set(rl.FIELDS) if name in dc.HAS_FIELD else {None})
    again = dc.make_draws(name)
    assert [_identity(d) for d in again] == [_identity(d) for d in draws]
    other = dc.NAMES[(dc.NAMES.index(name) + 1) % len(dc.NAMES)]
    assert _identity(dc.make_draws(other, count=1)[0])[1] != _identity(draws[0])[1]      # a generator of its own
    assert _identity(dc.make_draws(name, seed=dc.SEED + 1, count=1)[0])[1] != _identity(draws[0])[1]
    with pytest.raises(ValueError):                                  # accept() is the rule function: it refuses what the rules refuse
        bad = dict(draws[0].kw)
        bad[{"fold": "bucket", "hist": "bucket", "bands": "bands", "mask": "lo", "harm": "order", "rank": "lo", "cfar": "guard"}.get(name, "k")] = -1
        dc.accept(name, draws[0].field, bad)
    assert frames.FFT_SIZE == N


@pytest.mark.parametrize("name", dc.NAMES)
def test_the_draws_launch_every_kernel_instantiation(name):
    rl.built(name)
    inventory = ki.inventory(rl.lib_path(name))
    got = launched(name, dc.draws(name))
    assert got == inventory, (sorted(inventory - got), sorted(got - inventory))
    assert got != inventory | {f"{name}_dummy_kernel<3>"}            # a kernel form nobody draws breaks the equality
    few = launched(name, dc.draws(name)[:1])
    assert few != inventory and few < inventory                      # and so does an instantiation no draw reaches


@pytest.mark.parametrize("name", dc.NAMES)
def test_every_kind_is_reached(name):
    draws, wants = dc.draws(name), dc.wanted(name)
    count = reached(name, draws, wants)
    assert set(count) == set(dc.KINDS[name])
    low = {k: n for k, n in count.items() if n < LEAST}
    assert not low, (name, low)
    # the count is of draws: without the draws that reach the rarest kind, that kind is missed
    rare = min(count, key=count.get)
    kept = [(d, w) for d, w in zip(draws, wants) if rare not in dc.kinds(name, d, w)]
    assert len(kept) == dc.D - count[rare] and reached(name, *zip(*kept))[rare] == 0


@pytest.mark.parametrize("name", dc.NAMES)
def test_the_comparer_is_not_blind(name):
    """Every plain array of the result -- each field of a structured one -- with one bit of one element flipped: compare() says
    so.  The element is the first that is no NaN (a NaN's payload has no meaning in some arrays); an array that is empty in
    one draw (cross without fractions) is flipped in the next that has it."""
    seen = set()
    labels = None
    for d, want in zip(dc.draws(name), dc.wanted(name)):
        assert dc.compare(name, want, want) is None and dc.compare(name, copy.deepcopy(want), want) is None
        here = [label for label, _ in dc.plain_arrays(want)]
        labels = here if labels is None else labels
        assert here == labels
        for i, label in enumerate(labels):
            if label in seen:
                continue
            got = copy.deepcopy(want)
            a = dc.plain_arrays(got)[i][1]
            ok = np.argwhere(~np.isnan(a)) if a.dtype.kind == "f" else np.argwhere(np.ones(a.shape, bool))
            if not len(ok):
                continue
            at = tuple(ok[len(ok) // 2])
            a.view(f"u{a.dtype.itemsize}")[at] ^= 1
            bad = dc.compare(name, got, want)
            assert bad is not None, (name, label, at)
            assert dc.compare(name, got[:-1], want) is not None       # an array left out is seen too
            seen.add(label)
        if len(seen) == len(labels):
            break
    assert labels and seen == set(labels), (name, sorted(set(labels) - seen))
    assert dc.compare(name, want[:-1] + (want[-1][..., :0],), want) is not None         # a shape is part of the result


def test_a_failure_names_its_draw_in_one_line():
    for name in dc.NAMES:
        for d in (dc.draws(name)[0], dc.draws(name)[dc.D - 1]):
            line = dc.show(name, d)
            assert "\n" not in line and f"library {name}, draw {d.index}:" in line and dc.METHODS[name] in line
            assert all(f"{k}=" in line for k in d.kw)
