"""GPU: every call form once at byte offsets past 2^31 and 2^32, all rows compared.  tests/offset_cases.py is the table (one
case per call, input form, out kind and kernel it is there to reach) and tests/test_offset_cases_cpu.py its guard.

A case.  One period of P signal-carrying rows is drawn on the device from a seeded generator and tiled to B rows (a stream:
one period of P * hop samples, so that frame f is frame f mod P); B is the smallest batch at which the last row of the
call's smallest spectrum-sized tensor starts at or beyond byte 2^32, plus two rows.  The reference is the same call on the
first P rows alone -- small batches are held to the oracles and mirrors by the other files, and P > 512 launches the kernel
forms of the large call -- and must itself be non-zero, finite and pairwise different row by row, or the test fails as
vacuous.  The large call writes into an `out` filled with 0xFF bytes; then every whole period of `out` equals the reference
by bits, and the tail its head: all B rows (B / A groups), not a sample, so a store that wrapped onto any row shows.  A
wrong offset may also show as a memory fault: its cause is then in the address arithmetic of the kernels the case names.

The calls of the nine reduction libraries go through one path, gpu_support.ReductionCall on the arguments of the table: every
output of drawn_cases.outputs that has a row per row is compared so, a threshold per row is tiled like the input, and rows of
the reference are held to the numpy mirror (drawn_cases.compare)."""
import numpy as np
import pytest

import drawn_cases as dc
import offset_cases as oc
import structured_cases
from gpu_support import ReductionCall, ch, torch_mod  # noqa: F401 (fixtures)
from fpga_real_time_fft_analyzer_amd import chain
from offset_cases import CASES, N, TWO32
from q15_cases import configure as configure_q15

pytestmark = pytest.mark.gpu

I16_SCALE = 1.0 / 2048
MERGED = "level_hist-mag-group=all"


def _input_key(case):
    """Cases with one key read prefixes of one tiled input."""
    return (case.form, case.hop or 0, case.P, case.id == MERGED, case.recipe)


ORDERED = sorted(CASES, key=lambda c: (_input_key(c), c.B))
_held = {}                      # at most one tiled input at a time: key -> (tensor, frames it holds)


def _elements(case, B):
    """Elements of the input of B frames along its first axis: B rows, or the stream that ends with frame B - 1."""
    _, stream, row = oc.FORMS[case.form]
    return (B - 1) * (row[0] * case.hop // N) + row[0] if stream else B


def _one_period(torch, case):
    """P rows of signal (a stream: P * hop samples) from a generator seeded by the input form."""
    dtype, stream, row = oc.FORMS[case.form]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242 + sorted(oc.FORMS).index(case.form) + (case.hop or 0))
    P = case.P
    if stream:
        n = P * (row[0] * case.hop // N)
        return (torch.randint(-2048, 2048, (n,), dtype=torch.int16, device="cuda", generator=gen) if dtype == "int16"
                else torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen))
    if case.form == "f32":                                          # a tone per frame plus noise
        f = 0.01 + 0.44 * torch.rand((P, 1), device="cuda", generator=gen)
        t = torch.arange(N, device="cuda", dtype=torch.float32)
        return 0.8 * torch.sin(2 * np.pi * f * t) + 0.05 * torch.randn((P, N), device="cuda", generator=gen)
    if case.form == "i16":                                          # the 12-bit draw of q15_cases
        return torch.randint(-2048, 2048, (P, N), dtype=torch.int16, device="cuda", generator=gen)
    if case.form == "p12":                                          # every byte pattern is two packed 12-bit samples
        return torch.randint(0, 256, (P,) + row, dtype=torch.uint8, device="cuda", generator=gen)
    if case.form == "iq":
        return torch.randint(-32768, 32768, (P, N, 2), dtype=torch.int16, device="cuda", generator=gen)
    # magnitudes and records: non-negative and, without a recipe, all below the top edge of the histogram; a plant sets both
    # floats of a record
    noise, plants = oc.RECIPES[case.recipe] if case.recipe else ("uniform", ())
    u = torch.rand((P,) + row, device="cuda", generator=gen)
    per = 0.001 + 0.78 * u if noise == "uniform" else torch.exp(8.0 * u - 4.0)
    r = torch.arange(P, device="cuda")
    for first, step, width, value in plants:
        per[r, first + step * r + (1 + r % width if width else 0)] = value
    return per


def _tiled_input(torch, case):
    """The input of `case`: a prefix of the tiled tensor its key shares, built when the key changes."""
    key = _input_key(case)
    if key not in _held:
        _held.clear()
        torch.cuda.empty_cache()
        frames = max(c.B for c in CASES if _input_key(c) == key)
        per = _one_period(torch, case)
        x = torch.empty((_elements(case, frames),) + tuple(per.shape[1:]), dtype=per.dtype, device="cuda")
        for s in range(0, x.shape[0], per.shape[0]):
            n = min(per.shape[0], x.shape[0] - s)
            x[s:s + n] = per[:n]
        _held[key] = x
    return _held[key][:_elements(case, case.B)]


def _sentinel(torch, shape, dtype):
    """A tensor of that shape and dtype whose every byte is 0xFF."""
    raw = torch.full((int(np.prod(shape)) * oc.ITEMSIZE[oc._torch_name(dtype)],), 0xFF, dtype=torch.uint8, device="cuda")
    if dtype == torch.complex64:
        return torch.view_as_complex(raw.view(torch.float32).view(tuple(shape) + (2,)))
    return raw.view(dtype).view(tuple(shape))


def _configure(ch, case):
    table = oc.chain_table(case)
    if table == "FLOAT_CHAIN":
        mode, casc = oc.FLOAT_SETUPS[case.setup]
        if casc is not None:
            ch.load_sos(structured_cases.cascades()[casc])
        ch.set_filter_mode(mode)
        ch.set_precision(case.precision)
    elif case.setup is not None:
        configure_q15(ch, case.setup)


def _chain_call(ch, case, x, out):
    """The call of a case that has a chain table on x into out; the tensor it returned."""
    if case.call == "process_f32":
        return ch.process_f32(x, out=out, out_kind=case.kind, scale=I16_SCALE)
    if case.call == "markers":
        ch.markers(x, out=out, scale=I16_SCALE)
        return out
    if case.call == "process_q15":
        return ch.process_q15(x, out=out, out_kind=case.kind, hop=case.hop)
    if case.call == "traces_q15":
        w, a = case.kind if isinstance(case.kind, tuple) else (case.kind, None)
        return ch.traces_q15(x, bucket=w, out=out, hop=case.hop, group=a)
    if case.call == "spectra_q15":
        return ch.spectra_q15(x, case.kind, out=out, hop=case.hop)
    if case.call == "fold_iq_q15":
        return ch.fold_iq_q15(x, case.kind, out=out)
    assert case.call == "filter_q15", case.call
    return ch.filter_q15(x, out)


def _make(torch, ch, case, x, frames):
    """The call of the case on x, `frames` frames, every output 0xFF bytes before it: (name of offset_cases.tensors -> each
    tensor it wrote that has a row per row, the ReductionCall of a handle-free call or None)."""
    if case.call in oc.LIBRARY:
        name, field, kw = oc.arguments(case, frames)
        call = ReductionCall(torch, name, x, field, kw).launch(ch)
        wrote = {arg: raw.view(getattr(torch, dtype)).view(shape) for arg, (raw, shape, dtype) in call.held.items()}
        wrote.update({arg: call.returned[i] for arg, i, _ in dc.RETURNED.get(name, ())})
        return {k: wrote[k] for k in oc.tensors(case) if k in wrote}, call
    shape, dtype = chain.output_spec(getattr(chain, oc.chain_table(case)), case.kind, frames)
    out = _sentinel(torch, shape, dtype)
    assert _chain_call(ch, case, x, out).data_ptr() == out.data_ptr()
    return {"out": out}, None


# what the reference of a library must hold beside non-zero, different rows, from the result in the form of
# drawn_cases.mirror() and `at`, the place of the first plant of the recipe in every row: crossings reached at many bins;
# rows that fail and rows that pass, the worst bin at many places; the fundamental found at the row's own place; three
# segments, the first at the row's own place; the carrier the strongest ratio of its row
NOT_VACUOUS = {
    "bands": lambda got, at: bool((got[1] >= 0).all()) and np.unique(got[1][:, 0, 0]).size > 8,
    "mask": lambda got, at: (0 < int(((got[0]["over"] > 0) | (got[0]["under"] > 0)).sum()) < len(got[0])
                             and np.unique(got[0]["up_bin"]).size > 8),
    "harm": lambda got, at: got[0]["bin"][:, 0].tolist() == at.tolist(),
    "signals": lambda got, at: got[1][:, 0].tolist() == [3] * len(at) and got[0]["start"][:, 0].tolist() == at.tolist(),
    "cfar": lambda got, at: got[0].argmax(axis=1).tolist() == at.tolist(),
}


def _reference_is_the_mirrors(case, x, call):
    """The one-period reference of a handle-free case, on the host in the form of drawn_cases.mirror(): its floats finite, the
    library's own predicate, and the rows (groups) 0, 1, the last and the one the last row of the large call repeats equal
    to the numpy mirror by drawn_cases.compare.  An array the call has one of (the mask summary) is no row of anything: the
    mirror's own stands in its place here and test_mask_summary_past_4_gib holds it."""
    P, A = case.P, case.A
    got = call.result()
    for label, a in dc.plain_arrays(got):
        assert a.dtype.kind != "f" or bool(np.isfinite(a).all()), (case.id, label, "a reference row is not finite")
    name = oc.LIBRARY[case.call]
    if name in NOT_VACUOUS:
        first, step = oc.RECIPES[case.recipe][1][0][:2] if case.recipe else (0, 0)
        assert NOT_VACUOUS[name](got, first + step * np.arange(P)), (case.id, "the reference says nothing")
    groups = sorted({0, 1, P // A - 1, (case.B // A - 1) % (P // A)})
    _, field, kw = oc.arguments(case, P, only=groups)
    host = x[[g * A + i for g in groups for i in range(A)]].cpu().numpy()
    want = dc.mirror(name, host if field is None else np.ascontiguousarray(host[..., dc.FIELDS.index(field) - 1]), field, kw)
    some = tuple(g[groups] if g.shape[0] == P // A else w for g, w in zip(got, want))
    bad = dc.compare(name, some, want)
    assert bad is None, (case.id, groups, bad)
    return got


def _floating(torch, case, t):
    """The floating-point content of an output, or None where it has none."""
    if case.kind == "marker":
        f = t.view(torch.float32)
        return f[:, [0, 2]] if oc.chain_table(case) == "FLOAT_CHAIN" else f[:, 0]
    if t.dtype == torch.complex64:
        return torch.view_as_real(t)
    return t if t.dtype == torch.float32 else None


def _last_row_offset(case, t, rows):
    """Bytes from the start of tensor `t` of `rows` rows to its last row, by data_ptr arithmetic."""
    return t[t.shape[0] - t.shape[0] // rows:].data_ptr() - t.data_ptr()


SUMMARY = [c.id for c in ORDERED if c.call == "mask_test"]        # one record per call beside the rows: a test of their own


def _every_row(ch, torch, cid):
    """One case of offset_cases.CASES: the reference on one period, the call on B rows into 0xFF bytes, every row of every
    output compared.  Returns the reference of a handle-free case on the host, in the form of drawn_cases.mirror(), and the
    host copy of every output of the large call that has no row per row."""
    case = oc.BY_ID[cid]
    P, B, A = case.P, case.B, case.A
    fig = oc.tensors(case)
    torch.cuda.reset_peak_memory_stats()
    x = _tiled_input(torch, case)
    _configure(ch, case)
    # the table's figures are the tensors' own: the last row (group) of the input, and of every output that reaches 2^32
    stream = oc.FORMS[case.form][1]
    first_of_last = _elements(case, B - A + 1) - (oc.FORMS[case.form][2][0] if stream else 1)
    assert x[first_of_last:].data_ptr() - x.data_ptr() == oc.last_row_start(*fig["in"]) >= 1 << 32
    decides = oc.deciding_tensor(case)[0]
    # the reference: the same call on the first P rows alone
    ref, ref_call = _make(torch, ch, case, x[:_elements(case, P)], P)
    refs = {k: oc.as_rows(torch, t, P // A).clone() for k, t in ref.items()}
    first = next(iter(refs))
    why = oc.vacuous(torch, refs[first], None if ref_call else _floating(torch, case, ref[first]))
    assert why is None, (cid, why)
    for k, _, _ in dc.RETURNED.get(oc.LIBRARY.get(case.call), ()):     # the candidate counts of the peak table: two rows may agree
        assert bool((refs[k] != 0).all()) and torch.unique(refs[k]).numel() > 1, (cid, k)
    held = _reference_is_the_mirrors(case, x, ref_call) if ref_call else None
    # the call
    got, call = _make(torch, ch, case, x, B)
    assert list(got) == list(refs) and (decides == "in" or decides in got)
    for k, t in got.items():
        if oc.last_row_start(*fig[k]) >= 1 << 32:
            assert _last_row_offset(case, t, B // A) == oc.last_row_start(*fig[k]), (cid, k)
        bad = oc.tiled_mismatch(torch, oc.as_rows(torch, t, B // A), refs[k])
        assert bad is None, (cid, k, tuple(t.shape), bad)
    torch.cuda.synchronize()
    once = {} if call is None else {k: raw.view(getattr(torch, dtype)).cpu().numpy() for k, (raw, _, dtype) in call.held.items()
                                    if k not in got}
    print(f"FIGURE {cid}: B {B} P {P}, " + ", ".join(f"{k} {rb * n} B" for k, (rb, n) in fig.items())
          + f"; all {B // A} rows equal row mod {P // A}; peak torch memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    del got, call, ref, ref_call, refs, x
    torch.cuda.empty_cache()
    return held, once


@pytest.mark.parametrize("cid", [c.id for c in ORDERED if c.id != MERGED and c.id not in SUMMARY])
def test_every_row_past_4_gib(ch, torch_mod, cid):
    """One case of offset_cases.CASES: the reference on one period, the call on B rows into 0xFF bytes, every row compared."""
    _every_row(ch, torch_mod, cid)


@pytest.mark.parametrize("cid", SUMMARY)
def test_mask_summary_past_4_gib(ch, torch_mod, cid):
    """A mask case: every row as in test_every_row_past_4_gib, and the summary, one record per call that tiling cannot check,
    in closed form from the records of one period: the rows over and the rows under are (whole periods) x the count of one
    period + the count of the tail, then the first and the last failing row -- of the call on one period and of the call on B."""
    (rec, one_period), once = _every_row(ch, torch_mod, cid)
    case = oc.BY_ID[cid]
    P = case.P
    over, under = rec["over"] > 0, rec["under"] > 0
    fails = np.nonzero(over | under)[0].tolist()

    def summary(rows):
        whole, tail = divmod(rows, P)
        return [whole * int(over.sum()) + int(over[:tail].sum()), whole * int(under.sum()) + int(under[:tail].sum()), fails[0],
                max(f + P * (whole if f < tail else whole - 1) for f in fails)]

    assert one_period.tolist() == summary(P), cid
    assert once["summary"].tolist() == summary(case.B), cid


def test_merged_histogram_past_4_gib(ch, torch_mod):
    """level_hist with one group of all B rows (B odd: eight row slices of unequal length that merge into a zeroed output)
    merges rows, so tiling alone cannot show a wrapped read: the rows that start at or beyond 2^32 hold a constant above the
    top edge and every other point lies below it.  The counts are (B // P) x the counts of one period as one group + the
    counts of the tail as one group, in integers, and the top level is (rows past 2^32) x W in every column."""
    torch = torch_mod
    case = oc.BY_ID[MERGED]
    P, B, W = case.P, case.B, case.params["bucket"]
    L = len(oc.HIST_EDGES) + 1
    x = _tiled_input(torch, case)
    past = B - TWO32 // (N * 4)
    assert past == 1 + oc.EXTRA and x[B - past:].data_ptr() - x.data_ptr() == 1 << 32
    assert float(x.max()) < oc.HIST_EDGES[-1]
    x[B - past:] = oc.HIST_ABOVE
    period = ch.level_hist(x[:P], oc.HIST_EDGES, group=None, bucket=W).to(torch.int64)
    tail = ch.level_hist(x[B // P * P:].clone(), oc.HIST_EDGES, group=None, bucket=W).to(torch.int64)
    name, field, kw = oc.arguments(case, P)                             # the period as one group equals the numpy mirror
    bad = dc.compare(name, (period.to(torch.uint32).cpu().numpy(),), dc.mirror(name, x[:P].cpu().numpy(), field, kw))
    assert bad is None, bad
    assert tuple(period.shape) == (1, N // W, L) and bool((period[..., :L - 1] > 0).all()) and not bool(period[..., L - 1].any())
    assert bool((period.sum(dim=2) == P * W).all()) and bool((tail[..., L - 1] == past * W).all())
    out = _sentinel(torch, (1, N // W, L), torch.uint32)
    got = ch.level_hist(x, oc.HIST_EDGES, group=None, bucket=W, out=out).to(torch.int64)
    want = (B // P) * period + tail
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert bool((got[..., L - 1] == past * W).all()) and bool((got.sum(dim=2) == B * W).all())
    print(f"FIGURE {MERGED}: B {B} P {P}, in {B * N * 4} B; {past} rows past 2^32 counted in the top level of every column")
    del out, got, x
    _held.clear()
    torch.cuda.empty_cache()
