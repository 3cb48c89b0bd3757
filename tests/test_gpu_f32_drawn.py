"""GPU: the nine handle-free reduction libraries on DRAWN rows and arguments (tests/drawn_cases.py), through the SpectrumChain
method of each -- fold_mag_f32, find_peaks, order_stats, level_hist, band_power, mask_test, harmonics, find_signals, cfar.

Every comparison is drawn_cases.compare against the numpy mirror of frames.py: bits on integer views, every output of the
call, a NaN by position only where the library's own file compares it so.  The rows and arguments of tests/test_gpu_f32_x.py
were placed by hand at the seams their author knew; these are D = 96 draws per library of a fixed seed, which
tests/test_drawn_cases_cpu.py holds to launching every kernel instantiation and to reaching every kind of outcome.  Every
output given through ``out=`` starts as 0xFF bytes, so that a word the kernel does not write shows.

A failure names the library, the draw and its arguments in one line (drawn_cases.show): the draws are those of the seed, so
that line repeats it."""
import gc

import numpy as np
import pytest

import drawn_cases as dc
from conftest import N
from gpu_support import ReductionCall, ch, to_device, torch_mod  # noqa: F401 (fixtures)
from reduction_libraries import records_of
from test_gpu_f32_peaks import _inputs, _tones

pytestmark = pytest.mark.gpu


def _call_of(torch, name, d, x=None):
    return ReductionCall(torch, name, to_device(torch, records_of(d.pts, d.field)) if x is None else x, d.field, d.kw)


def _bad(name, draw, got, want):
    bad = dc.compare(name, got, want)
    return None if bad is None else f"{dc.show(name, draw)}: {bad}"


@pytest.mark.parametrize("name", dc.NAMES)
def test_drawn_calls_equal_the_mirror(ch, torch_mod, name):
    """Each of the D draws, one call at a time: every output equals the mirror's."""
    for d, want in zip(dc.draws(name), dc.wanted(name)):
        bad = _bad(name, d, _call_of(torch_mod, name, d).launch(ch).result(), want)
        assert bad is None, bad


@pytest.mark.parametrize("name", dc.NAMES)
def test_queued_drawn_calls(ch, torch_mod, name):
    """All D inputs, device arguments and outputs resident, then all D calls on the current stream with nothing between them
    -- no copy, no allocation of the test's, no wait -- every object that held an argument dropped as its call returns, then
    one synchronisation: every result equals the mirror's.  The edges, bands, fractions, ranks and limits of a call are gone
    from the host before its kernel has to have run, and each kernel meets the LDS a differently parameterised launch of
    itself left."""
    torch = torch_mod
    draws = dc.draws(name)
    calls = [_call_of(torch, name, d) for d in draws]
    torch.cuda.synchronize()
    for c in calls:
        c.launch(ch)
    gc.collect()
    torch.cuda.synchronize()
    for d, want, c in zip(draws, dc.wanted(name), calls):
        bad = _bad(name, d, c.result(), want)
        assert bad is None, bad


def test_interleaved_libraries(ch, torch_mod):
    """The first 24 draws of every library, round robin across the nine on one stream, one synchronisation at the end: each
    kernel starts on the LDS another library's kernel left."""
    torch = torch_mod
    calls = [(name, d, _call_of(torch, name, d)) for i in range(24) for name in dc.NAMES for d in [dc.draws(name)[i]]]
    assert len(calls) == 24 * 9 and [name for name, _, _ in calls[:9]] == list(dc.NAMES)
    torch.cuda.synchronize()
    for _, _, c in calls:
        c.launch(ch)
    gc.collect()
    torch.cuda.synchronize()
    for name, d, c in calls:
        bad = _bad(name, d, c.result(), dc.wanted(name)[d.index])
        assert bad is None, bad


def test_drawn_rows_at_a_row_offset(ch, torch_mod):
    """8 draws of each library whose input is the rows [r0, r0 + R) of a larger tensor of NaNs, r0 drawn: the result is the
    mirror's -- a NaN read from a row around the slice would show in it -- and the rows around the slice stay what they were."""
    torch = torch_mod
    for name in dc.NAMES:
        rng = np.random.default_rng([dc.SEED, len(dc.NAMES), dc.NAMES.index(name)])
        short = [d for d in dc.draws(name) if d.pts.shape[0] <= 8]
        for d in [short[int(i)] for i in rng.choice(len(short), 8, replace=False)]:
            x = records_of(d.pts, d.field)
            R, r0, after = x.shape[0], int(rng.integers(1, 6)), int(rng.integers(1, 4))
            big = torch.full((r0 + R + after,) + x.shape[1:], float("nan"), dtype=torch.float32, device="cuda")
            big[r0:r0 + R] = to_device(torch, x)
            before = big.view(torch.int32).clone()
            bad = _bad(name, d, _call_of(torch, name, d, big[r0:r0 + R]).launch(ch).result(), dc.wanted(name)[d.index])
            assert bad is None, (r0, bad)
            assert torch.equal(big.view(torch.int32), before), (r0, dc.show(name, d))


def _composed_arguments(name, kw):
    """The arguments of the composed call that stands for the plain call with ``kw``: the same, but that noise_floor_f32 takes
    quantiles -- those whose ranks (frames.rank_of_quantile) are the drawn ones."""
    from fpga_real_time_fft_analyzer_amd import frames
    if name != "rank":
        return dict(kw)
    m = kw["hi"] - kw["lo"]
    q = [1.0 if r == m - 1 else (r + 0.5) / (m - 1) for r in kw["ranks"]]
    assert [frames.rank_of_quantile(v, m) for v in q] == list(kw["ranks"]), kw
    return dict(q=q, lo=kw["lo"], hi=kw["hi"])


def test_composed_calls_on_drawn_arguments(ch, torch_mod):
    """One batch of 4 int16 frames of three tones plus noise -- rows the chain really produces -- and the first 8 drawn
    argument sets of each library, field None: the composed call on the frames equals the plain call on
    process_f32(..., out_kind='mag_full') of the same frames byte for byte, and the plain call equals the mirror on those
    magnitudes.  Of fold and hist the first 8 sets whose group divides the 4 frames; a threshold per row is cut or repeated
    to 4 rows."""
    torch = torch_mod
    ch.set_filter_mode(0xB1)
    B = 4
    x = _inputs(torch, _tones(B, dc.SEED))["int16"]
    mag = ch.process_f32(x, out_kind="mag_full").clone()
    rows = mag.cpu().numpy()
    assert rows.shape == (B, N) and np.isfinite(rows).all() and (rows.max(axis=1) > 100 * np.median(rows, axis=1)).all()
    for name in dc.NAMES:
        sets = [d for d in dc.draws(name) if B % (d.kw.get("group") or B) == 0][:8]
        assert len(sets) == 8
        for d in sets:
            kw = dict(d.kw)
            if isinstance(kw.get("threshold"), np.ndarray):
                kw["threshold"] = np.resize(kw["threshold"], B)
            plain = ReductionCall(torch, name, mag, None, kw).launch(ch)
            composed = ReductionCall(torch, name, x, None, kw, composed=_composed_arguments(name, kw)).launch(ch)
            for arg in plain.held:
                assert torch.equal(composed.held[arg][0], plain.held[arg][0]), (arg, dc.show(name, d))
            if name == "peaks":
                assert torch.equal(composed.returned[2], plain.returned[2]), dc.show(name, d)
            bad = _bad(name, d, plain.result(), dc.mirror(name, rows, None, kw))
            assert bad is None, bad
