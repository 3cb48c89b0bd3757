"""GPU: every call form once at byte offsets past 2^31 and 2^32, all rows compared.  tests/offset_cases.py is the table (one
case per call, input form, out kind and kernel it is there to reach) and tests/test_offset_cases_cpu.py its guard.

A case.  One period of P signal-carrying rows is drawn on the device from a seeded generator and tiled to B rows (a stream:
one period of P * hop samples, so that frame f is frame f mod P); B is the smallest batch at which the last row of the
call's smallest spectrum-sized tensor starts at or beyond byte 2^32, plus two rows.  The reference is the same call on the
first P rows alone -- small batches are held to the oracles and mirrors by the other files, and P > 512 launches the kernel
forms of the large call -- and must itself be non-zero, finite and pairwise different row by row, or the test fails as
vacuous.  The large call writes into an `out` filled with 0xFF bytes; then every whole period of `out` equals the reference
by bits, and the tail its head: all B rows (B / A groups), not a sample, so a store that wrapped onto any row shows.  A
wrong offset may also show as a memory fault: its cause is then in the address arithmetic of the kernels the case names."""
import numpy as np
import pytest

import offset_cases as oc
import structured_cases
from gpu_support import ch, torch_mod  # noqa: F401 (fixtures)
from fpga_real_time_fft_analyzer_amd import chain
from offset_cases import CASES, N, TWO32
from q15_cases import configure as configure_q15

pytestmark = pytest.mark.gpu

I16_SCALE = 1.0 / 2048
MERGED = "level_hist-mag-group=all"


def _input_key(case):
    """Cases with one key read prefixes of one tiled input."""
    return (case.form, case.hop or 0, case.P, case.id == MERGED)


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
    # magnitudes and records: non-negative, all below the top edge of the histogram
    return 0.001 + 0.78 * torch.rand((P,) + row, device="cuda", generator=gen)


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


def _out_spec(case, B):
    table = oc.chain_table(case)
    if table is not None:
        return chain.output_spec(getattr(chain, table), case.kind, B)
    import torch
    p, R = case.params, B // case.A
    if case.call == "fold_mag_f32":
        return (R, N // p["bucket"], 2), torch.float32
    if case.call == "find_peaks":
        return (R, p["k"], 2), torch.int32
    if case.call == "order_stats":
        return (R, len(p["ranks"])), torch.float32
    return (1 if p["group"] is None else R, N // p["bucket"], len(oc.HIST_EDGES) + 1), torch.uint32


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


def _call(ch, case, x, out):
    """The call of the case on x into out; the tensors it wrote."""
    p = case.params
    if case.call == "process_f32":
        return (ch.process_f32(x, out=out, out_kind=case.kind, scale=I16_SCALE),)
    if case.call == "markers":
        ch.markers(x, out=out, scale=I16_SCALE)
        return (out,)
    if case.call == "process_q15":
        return (ch.process_q15(x, out=out, out_kind=case.kind, hop=case.hop),)
    if case.call == "traces_q15":
        w, a = case.kind if isinstance(case.kind, tuple) else (case.kind, None)
        return (ch.traces_q15(x, bucket=w, out=out, hop=case.hop, group=a),)
    if case.call == "spectra_q15":
        return (ch.spectra_q15(x, case.kind, out=out, hop=case.hop),)
    if case.call == "fold_iq_q15":
        return (ch.fold_iq_q15(x, case.kind, out=out),)
    if case.call == "filter_q15":
        return (ch.filter_q15(x, out),)
    if case.call == "fold_mag_f32":
        return (ch.fold_mag_f32(x, p["group"], p["bucket"], out=out),)
    if case.call == "find_peaks":
        return (out, ch.find_peaks(x, k=p["k"], field=p["field"], out=out)[2])
    if case.call == "order_stats":
        return (ch.order_stats(x, p["ranks"], field=p["field"], out=out),)
    assert case.call == "level_hist"
    return (ch.level_hist(x, oc.HIST_EDGES, group=p["group"], bucket=p["bucket"], out=out),)


def _floating(torch, case, t):
    """The floating-point content of an output, or None where it has none."""
    if case.kind == "marker":
        f = t.view(torch.float32)
        return f[:, [0, 2]] if oc.chain_table(case) == "FLOAT_CHAIN" else f[:, 0]
    if case.call == "find_peaks":
        return t.view(torch.float32)[..., 0] if t.dim() == 3 else None
    if t.dtype == torch.complex64:
        return torch.view_as_real(t)
    return t if t.dtype == torch.float32 else None


def _last_row_offset(case, t, rows):
    """Bytes from the start of tensor `t` of `rows` rows to its last row, by data_ptr arithmetic."""
    return t[t.shape[0] - t.shape[0] // rows:].data_ptr() - t.data_ptr()


@pytest.mark.parametrize("cid", [c.id for c in ORDERED if c.id != MERGED])
def test_every_row_past_4_gib(ch, torch_mod, cid):
    """One case of offset_cases.CASES: the reference on one period, the call on B rows into 0xFF bytes, every row compared."""
    torch = torch_mod
    case = oc.BY_ID[cid]
    P, B, A = case.P, case.B, case.A
    fig = oc.tensors(case)
    torch.cuda.reset_peak_memory_stats()
    x = _tiled_input(torch, case)
    _configure(ch, case)
    # the table's figures are the tensors' own: the last row (group) of the input, and of the output where that decides B
    stream = oc.FORMS[case.form][1]
    first_of_last = _elements(case, B - A + 1) - (oc.FORMS[case.form][2][0] if stream else 1)
    assert x[first_of_last:].data_ptr() - x.data_ptr() == oc.last_row_start(*fig["in"]) >= 1 << 32
    decides = oc.deciding_tensor(case)[0]
    # the reference: the same call on the first P rows alone
    shape, dtype = _out_spec(case, P)
    ref = _call(ch, case, x[:_elements(case, P)], _sentinel(torch, shape, dtype))
    refs = []
    for i, t in enumerate(ref):
        rows = oc.as_rows(torch, t, P // A).clone()
        if i == 0:
            why = oc.vacuous(torch, rows, _floating(torch, case, t))
            assert why is None, (cid, why)
        else:                                                       # the candidate counts of the peak table: two rows may agree
            assert bool((rows != 0).all()) and torch.unique(rows).numel() > 1, cid
        refs.append(rows)
    # the call
    shape, dtype = _out_spec(case, B)
    out = _sentinel(torch, shape, dtype)
    if decides == "out":
        assert _last_row_offset(case, out, B // A) == oc.last_row_start(*fig["out"]) >= 1 << 32
    got = _call(ch, case, x, out)
    assert got[0].data_ptr() == out.data_ptr()
    for t, want in zip(got, refs):
        bad = oc.tiled_mismatch(torch, oc.as_rows(torch, t, B // A), want)
        assert bad is None, (cid, tuple(t.shape), bad)
    torch.cuda.synchronize()
    print(f"FIGURE {cid}: B {B} P {P}, " + ", ".join(f"{k} {rb * n} B" for k, (rb, n) in fig.items())
          + f"; all {B // A} rows equal row mod {P // A}; peak torch memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    del out, got, ref, refs, x
    torch.cuda.empty_cache()


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
