"""Shared by tests/test_offset_cases_cpu.py (the guard) and tests/test_gpu_offsets.py (a plain module, like q15_cases.py: no
fixtures, importable without a GPU): the table of calls that are made once with a tensor whose last row starts at or beyond
byte 2^32, the bytes per row of every tensor such a call reads or writes, the kernels it launches and the comparison of a
tiled output with the output of one period.

Every kernel turns a frame or row index into a byte offset.  An offset computed in 32 bits is right for every batch the
other tests make; it wraps at 2^32 bytes (an unsigned) or turns negative at 2^31 (an int).  A case here makes the call at the
smallest batch at which such a defect can exist and compares EVERY row of the result, so that a store that wraps onto a row
nobody looked at is seen as well.

A case.  `call` is the SpectrumChain method; `form` the input (FORMS below); `kind` the out kind as the chain tables of
chain.py name it (traces_q15: the bucket W, with a group the pair (W, A); spectra_q15 / fold_iq_q15: A), None where the
call has one output; `setup` the filter setup -- a name of q15_cases.SETUPS for the integer chain, of FLOAT_SETUPS for the
float chain -- and `precision` that of the float chain; `A` the frames (rows) per output row; `hop` the stride of a stream
in samples; `params` the further arguments of a handle-free call.  `P` is the period of the input in rows and `B` the batch,
both made by the rules of period() and batch() and held to them, from the outside, by the guard; `recipe` names the rows of
one period (RECIPES), "" for the draw of the input form.

What a handle-free call is -- its method, its outputs, the kernels it launches, its mirror -- is said once, for all nine
reduction libraries, by tests/drawn_cases.py; its entry point is the one data-plane name of the library's signature table.

A tensor of a case is (bytes per row, rows): a row is what belongs to one output row, A frames where the call folds groups
of A frames.  Every byte count is derived from abi.py and chain.py (output_spec, the input forms' row lengths,
SA_P12_FRAME_BYTES); the one figure they do not hold, the 16 bytes of a partial record of the grouped trace, is held to
csrc/sa_common.hpp by the guard."""
import collections
import math
import re

import numpy as np

import drawn_cases as dc
import kernel_inventory as ki
import structured_cases
from fpga_real_time_fft_analyzer_amd import abi, chain

N = abi.SA_N
TWO31, TWO32 = 1 << 31, 1 << 32
EXTRA = 2                        # rows (groups) beyond the first whose start lies at or beyond 2^32; the rule allows up to 3
TRACE_RAW_RECORD_BYTES = 16      # kSaTraceRawBytes of csrc/sa_common.hpp (test_offset_cases_cpu.py reads it there)
# a tensor counts as spectrum-sized -- it decides B -- from one byte per bin on; the reduced outputs (marker records, peak
# tables, ranks, histograms of 64-bin columns) never reach 2^32 themselves: their inputs do
SPECTRUM_BYTES = N

# input form -> (torch dtype name, a 1-D stream cut at a hop?, elements of one frame or row)
FORMS = {"f32": ("float32", False, (N,)), "i16": ("int16", False, (N,)), "p12": ("uint8", False, (abi.SA_P12_FRAME_BYTES,)),
         "i16_hop": ("int16", True, (N,)), "p12_hop": ("uint8", True, (abi.SA_P12_FRAME_BYTES,)),
         "iq": ("int16", False, (N, 2)),          # fold_iq_q15: the IQ frames of process_q15
         "mag": ("float32", False, (N,)),         # the handle-free calls: rows of magnitudes ...
         "rec": ("float32", False, (N, 2))}       # ... or of {peak, power} records, read through `field`
ITEMSIZE = {"float32": 4, "int16": 2, "uint8": 1, "int32": 4, "uint32": 4, "complex64": 8}
HOPS = (16376, 16384)            # the largest stride below N (no power of two), and N itself

# float chain: name -> (filter byte, cascade of structured_cases.cascades() or None)
FLOAT_SETUPS = {"bypass": (0xB1, None), "default": (0x00, None),
                **{name: (0xA1, name) for name in structured_cases.CASCADE_VARIANTS}}
# integer chain: setup of q15_cases.SETUPS -> the cascade kernel it launches, as kernel_inventory.q15_kernels takes it
Q15_CASCADES = {"b1_rtl": None, "default": ("filter_q7", ("true",)), "wide6": ("filter_w14", ())}
# the calls of the float chain / of the integer chain, and their tables in chain.py
_Q15_TABLES = {"process_q15": "Q15_CHAIN", "filter_q15": "Q15_WINDOW_CHAIN", "spectra_q15": "Q15_SPECTRA_CHAIN",
               "fold_iq_q15": "Q15_FOLD_CHAIN"}
CHAIN_TABLES = ("FLOAT_CHAIN", "Q15_CHAIN", "Q15_TRACE_CHAIN", "Q15_TRACE_AVG_CHAIN", "Q15_WINDOW_CHAIN", "Q15_SPECTRA_CHAIN",
                "Q15_FOLD_CHAIN")
LIBRARY = {method: name for name, method in dc.METHODS.items()}      # the method of a handle-free call -> its library
HIST_EDGES = (0.2, 0.4, 0.6, 0.8)            # five levels; the data of the merged case stays below the top edge
HIST_ABOVE = 1.0                             # ... except the rows that start at or beyond 2^32, which hold this

# The rows of one period where the draw of the input form, 0.001 + 0.78 u, would leave a library's result without content:
# name -> (noise, plants).  Noise "uniform" is that draw, "exp" is exp(8 u - 4).  A plant (bin, step, width, value) sets the
# point `bin + step r` of row r -- a place of the row's own -- to `value`, with a width the point `1 + r % width` bins further.
RECIPES = {"tone": ("uniform", ((100, 7, 0, 5.0),)),                # harm: a fundamental per row
           # signals: three segments per row, each of the row's own place and width, above every threshold of the case
           "segments": ("uniform", tuple(p for j in range(3) for p in ((100 + 3000 * j, 7, 0, 5.0), (100 + 3000 * j, 7, 3, 6.0)))),
           "carrier": ("exp", ((100, 13, 0, 500.0),))}             # cfar: exponential noise, a carrier per row

Case = collections.namedtuple("Case", "id call form kind setup precision A hop params P B recipe")


# ------------------------------------------------------------------------------------------------------- bytes per row
def _table(call, kind):
    if call in ("process_f32", "markers"):
        return "FLOAT_CHAIN"
    if call == "traces_q15":
        return "Q15_TRACE_AVG_CHAIN" if isinstance(kind, tuple) else "Q15_TRACE_CHAIN"
    return _Q15_TABLES.get(call)


def chain_table(case):
    """The name of the chain table of chain.py a case's call goes through; None for a handle-free call."""
    return _table(case.call, case.kind)


def arguments(case, R, only=None):
    """(library, field, kw) of a handle-free case's call on R frames, as drawn_cases takes them: an argument of one entry per
    row of the period -- a threshold per row -- is tiled to the R rows like the input.  `only`: of those rows these alone."""
    return (LIBRARY[case.call],) + _arguments(case.params, case.P // case.A, R // case.A, only)


def _arguments(params, period_rows, rows, only=None):
    def tiled(v):
        v = np.resize(v, (rows,) + v.shape[1:])
        return v if only is None else v[list(only)]
    return params.get("field"), {k: tiled(v) if _per_row(v, period_rows) else v for k, v in params.items() if k != "field"}


def _per_row(v, period_rows):
    """No argument has a fixed extent of a period's rows (a limit line has N points)."""
    return isinstance(v, np.ndarray) and v.shape[0] == period_rows


def _prod(shape):
    return math.prod(shape)


def frame_stride_bytes(form, hop=None):
    """Bytes from one frame (row) of the input to the next: the frame itself, or at a hop `row * hop / 16384` elements, as
    chain.SpectrumChain._check_in steps through a stream."""
    dtype, stream, row = FORMS[form]
    if not stream:
        return _prod(row) * ITEMSIZE[dtype]
    return row[0] * hop // N * ITEMSIZE[dtype]


def input_bytes(form, hop, B):
    """The bytes the call reads through `x`: B frames, or the stream that ends with frame B - 1."""
    dtype, stream, row = FORMS[form]
    return (B - 1) * frame_stride_bytes(form, hop) + _prod(row) * ITEMSIZE[dtype]


def _torch_name(dtype):
    return str(dtype).replace("torch.", "")


def out_row_bytes(table, kind):
    """Bytes of one row of `out` of a call that has a chain table, from chain.output_spec."""
    ch = getattr(chain, table)
    per_row = ch.output(kind)[3]
    shape, dtype = chain.output_spec(ch, kind, per_row)
    assert shape[0] == 1
    return _prod(shape[1:]) * ITEMSIZE[_torch_name(dtype)]


def _handle_free_tensors(name, A, params):
    """The tensors beside the input that grow with the batch of a handle-free call: of drawn_cases.outputs those with one
    row per row -- no fixed extent (the 4 words of the mask summary, the 1 group of the merged histogram) equals the rows of
    a period --, what the method only returns, and an argument per row."""
    m = period(A) // A
    _, kw = _arguments(params, m, m)
    t = {arg: _prod(shape[1:]) * np.dtype(dtype).itemsize for arg, shape, dtype in dc.outputs(name, m * A, kw) if shape[0] == m}
    t.update({arg: np.dtype(dtype).itemsize for arg, _, dtype in dc.RETURNED.get(name, ())})
    t.update({k: v[0].nbytes for k, v in kw.items() if _per_row(v, m)})
    return t


def row_tensors(call, form, kind, setup, precision, A, hop, params):
    """name -> bytes per row of every tensor of the call that grows with the batch, a row being A frames: "in", the outputs by
    the names of their arguments ("out"; bands: "power" and "cross"; signals: "out", "stats" and the "threshold" per row; the
    "count" find_peaks returns), and the handle's workspaces -- "ws_q15" (the cascade's int16 frames in front of the FFT),
    "ws_f64" (the float64-state cascade's float32 frames in front of the bypassed chain), "ws_trace" (the partial records of
    the grouped trace), "ws_iq" (the IQ frames of spectra_q15).  The merged histogram (group None) is one output row of all
    B rows: its input is counted row by row and its output does not grow."""
    t = {"in": A * frame_stride_bytes(form, hop)}
    if call in LIBRARY:
        t.update(_handle_free_tensors(LIBRARY[call], A, params))
        return t
    t["out"] = out_row_bytes(_table(call, kind), kind)
    if call in ("process_f32", "markers") and precision == "f64" and kind != "time":
        t["ws_f64"] = A * N * ITEMSIZE["float32"]
    if call in ("process_q15", "traces_q15", "spectra_q15") and Q15_CASCADES[setup] is not None:
        t["ws_q15"] = A * N * ITEMSIZE["int16"]
    if call == "traces_q15" and isinstance(kind, tuple):
        t["ws_trace"] = A * (N // kind[0]) * TRACE_RAW_RECORD_BYTES
    if call == "spectra_q15":
        t["ws_iq"] = A * abi.SA_FRAME_BYTES
    return t


def tensors(case):
    """name -> (bytes per row, rows) of a case at its B."""
    return {k: (v, case.B // case.A) for k, v in row_tensors(*case[1:9]).items()}


def last_row_start(row_bytes, rows):
    return (rows - 1) * row_bytes


def deciding_tensor(case_or_rows):
    """The smallest spectrum-sized tensor of a call, (name, bytes per row): the one whose last row is the last to reach 2^32."""
    rows = case_or_rows if isinstance(case_or_rows, dict) else {k: v[0] for k, v in tensors(case_or_rows).items()}
    big = {k: v for k, v in rows.items() if v >= SPECTRUM_BYTES}
    name = min(big, key=lambda k: (big[k], k))
    return name, big[name]


def period(A):
    """P: a multiple of A above 512 (the one-round float kernel serves B <= 512) with an odd factor above 1, so that no power
    of two is a multiple of P x (bytes per row): 1027 at A = 1, A x an odd number for groups."""
    if A == 1:
        return 1027
    odd = (512 // A + 1) | 1
    assert odd > 1 and A * odd > 512
    return A * odd


def batch(rows, A):
    """B: the smallest batch at which the last row of the deciding tensor starts at or beyond 2^32, plus EXTRA rows."""
    _, row_bytes = deciding_tensor(rows)
    return (-(-TWO32 // row_bytes) + 1 + EXTRA) * A


def _case(call, form, kind=None, setup=None, precision=None, A=1, hop=None, recipe="", **params):
    if _table(call, kind) == "FLOAT_CHAIN":
        precision = precision or "f32"
    rows = row_tensors(call, form, kind, setup, precision, A, hop, params)
    words = [call, form + (str(hop) if hop else "")]
    words += ["x".join(map(str, kind)) if isinstance(kind, tuple) else str(kind)] if kind is not None else []
    words += [setup] if setup else []
    words += ["f64"] if precision == "f64" else []
    words += [f"{k}={'all' if v is None else v}" for k, v in params.items() if k in ("field", "group")]
    return Case("-".join(words), call, form, kind, setup, precision, A, hop, params, period(A), batch(rows, A), recipe)


def _cases():
    c = []
    # the float chain: every input type x every out kind (chain_f32_kernel x 3 OUT, chain_marker_kernel, time_f32_kernel), a
    # cascade in the unit-numerator form, the bypass, the general form; then iir_f64_kernel on every input type, whose
    # float32 frames go through a workspace -- with the smallest output, the marker
    for form, setup in (("f32", "butter12"), ("i16", "bypass"), ("p12", "default")):
        for kind in ("mag_full", "mag_half", "spec_half", "time"):
            c.append(_case("process_f32", form, kind, setup))
        c.append(_case("markers", form, "marker", setup))
    for form, setup in (("f32", "long_memory"), ("i16", "butter5_padded"), ("p12", "butter12")):
        c.append(_case("markers", form, "marker", setup, "f64"))
    # the integer chain without a cascade: the FFT reads the samples, in its four input forms x five OUT (iq, mag, marker,
    # trace, partial records); buckets 2 and 4 are the traces whose rows are 64 and 32 KiB; the grouped trace at bucket 2 on
    # int16 frames is the one whose partial records, 128 KiB per frame, pass 2^32 (17 GB of workspace: once is enough)
    for form, hop, w, wa in (("i16", None, 4, 2), ("p12", None, 2, 64), ("i16_hop", HOPS[0], 2, 64), ("p12_hop", HOPS[0], 4, 64)):
        for kind in ("iq", "mag", "marker"):
            c.append(_case("process_q15", form, kind, "b1_rtl", hop=hop))
        c.append(_case("traces_q15", form, w, "b1_rtl", hop=hop))
        c.append(_case("traces_q15", form, (wa, 2), "b1_rtl", A=2, hop=hop))
        c.append(_case("spectra_q15", form, 2, "b1_rtl", A=2, hop=hop))
    for form in ("i16_hop", "p12_hop"):                  # the stride N: f * hop and f * (3 * hop / 2) at a power of two
        c.append(_case("process_q15", form, "marker", "b1_rtl", hop=HOPS[1]))
    c.append(_case("traces_q15", "i16", (4, 2), "b1_rtl", A=2))      # the grouped trace's 32 KiB rows pass 2^32 here alone
    for form in ("i16", "p12"):                          # window_q15_kernel
        c.append(_case("filter_q15", form, None, "b1_rtl"))
    # behind a cascade the FFT reads int16 frames from the workspace, unwindowed: its five OUT on int16 frames; then each
    # cascade kernel in its other input forms, with the marker
    for kind in ("iq", "mag", "marker"):
        c.append(_case("process_q15", "i16", kind, "default"))
    c.append(_case("traces_q15", "i16", 16, "default"))
    c.append(_case("traces_q15", "i16", (64, 2), "default", A=2))
    for form, hop in (("p12", None), ("i16_hop", HOPS[0]), ("p12_hop", HOPS[0])):
        c.append(_case("process_q15", form, "marker", "default", hop=hop))
    for form, hop in (("i16", None), ("p12", None), ("i16_hop", HOPS[0]), ("p12_hop", HOPS[0])):
        c.append(_case("process_q15", form, "marker", "wide6", hop=hop))
    c.append(_case("fold_iq_q15", "iq", 2, A=2))
    # the handle-free calls: the float fold; the histogram with many groups (one slice) and with one group of all rows (row
    # slices that merge); the seven libraries that read records on magnitudes and on both fields of records.  bands with a
    # fraction, so that `cross` is written; mask with both limit lines -- the top and the bottom 0.03 % of the points lie
    # beyond them, so some rows fail and some pass -- and its summary; signals with a threshold per row; cfar's output is
    # spectrum-sized, so it decides B where the input rows are records
    c.append(_case("fold_mag_f32", "mag", A=2, group=2, bucket=1))
    c.append(_case("level_hist", "mag", A=2, edges=HIST_EDGES, group=2, bucket=64, lo=0, hi=N))
    c.append(_case("level_hist", "mag", edges=HIST_EDGES, group=None, bucket=64, lo=0, hi=N))
    rng = np.random.default_rng(2361)
    upper, lower = rng.uniform(0.7808, 0.7812, N).astype(np.float32), rng.uniform(0.0005, 0.0012, N).astype(np.float32)
    per_row = (2.0 + 0.25 * (np.arange(period(1)) % 5)).astype(np.float32)
    for a in (upper, lower, per_row):
        a.setflags(write=False)                                   # shared by three cases each
    for form, field in (("mag", None), ("rec", "peak"), ("rec", "power")):
        c.append(_case("find_peaks", form, field=field, k=8))
        c.append(_case("order_stats", form, field=field, ranks=(0, N // 2, N - 1)))
        c.append(_case("band_power", form, field=field, bands=[(100, 16000), (8191, 8450)], fracs=(0.5,)))
        c.append(_case("mask_test", form, field=field, upper=upper, lower=lower, lo=100, hi=16001))
        c.append(_case("harmonics", form, recipe="tone", field=field, order=10, span=3))
        c.append(_case("find_signals", form, recipe="segments", field=field, k=4, threshold=per_row, gap=3))
        c.append(_case("cfar", form, recipe="carrier", field=field, train=32, guard=3, mode="go", what="ratio", lo=1, hi=N - 1))
    return tuple(c)


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), sorted(c.id for c in CASES if [d.id for d in CASES].count(c.id) > 1)


# ------------------------------------------------------------------------------------------------- what a case launches
def data_plane(signatures):
    """The entry points of a signature table of abi.py that take data."""
    return {n for n in signatures if not re.search(r"_(version|check|last_error)$", n)}


def entry_point(case):
    """The C entry point the call goes to: of a handle-free call the one data-plane name of its library."""
    table = chain_table(case)
    if table is None:
        (name,) = data_plane(abi.LIBRARIES[LIBRARY[case.call]][1])
        return name
    ch = getattr(chain, table)
    forms = ch.streams if FORMS[case.form][1] else ch.inputs
    return {_torch_name(k): v for k, v in forms.items()}[FORMS[case.form][0]][1][case.kind][0]


def table_row(case):
    """(chain table, torch dtype, "stream" / "frames") of a call that has a chain table."""
    return chain_table(case), FORMS[case.form][0], "stream" if FORMS[case.form][1] else "frames"


def kernels(case):
    """The kernel instantiations a case launches, as kernel_inventory keys them."""
    if chain_table(case) == "FLOAT_CHAIN":
        mode, casc = FLOAT_SETUPS[case.setup]
        nsec, unit = (0, 0) if mode == 0xB1 else (6, 0) if casc is None else structured_cases.CASCADE_VARIANTS[casc][:2]
        f64 = case.precision == "f64"
        wingen = int(nsec > 0 and case.kind != "time" and not f64)         # the cosine window is generated behind a cascade
        return ki.float_kernels((FORMS[case.form][0], nsec, 0 if f64 else unit, wingen, False, case.kind, case.precision))
    if case.call == "fold_iq_q15":
        return ("spectra_fold_q15_kernel",)
    if chain_table(case) is not None:
        what = {"process_q15": case.kind, "filter_q15": "filter", "spectra_q15": "spectra",
                "traces_q15": "trace_avg" if isinstance(case.kind, tuple) else "trace"}[case.call]
        return ki.q15_kernels(Q15_CASCADES[case.setup], case.form, what)
    name, field, kw = arguments(case, case.B)
    return dc.kernels(name, case.B, field, kw)


# template arguments that do not enter an address, by kernel stem: their positions are dropped from a key
#   NSEC, UNIT, WINGEN: sections and window of the float cascade, arithmetic on a frame already in LDS
#   NOB1: the short or the long step of the Q7 cascade, the same
#   K of the float fold, STEPS of the histogram: the bucket's lane ladder and the depth of the edge tree; the row offsets
#   of both kernels are those of the one instantiation a case launches
#   UP, LOW of the mask test: whether fetch() of csrc/mask_f32.hip loads upper[q] and lower[q], q the 4-bin unit within a
#   row -- an index below N / 4 that the row never enters
#   CROSS of the band power: bands_f32_kernel<FIELD, true> makes every access of <FIELD, false> -- the reads of the row and
#   the store to power[row nb + j] stand outside `if constexpr (CROSS)` -- plus the store to cross[(row nb + j) nq + q], so
#   a case with a fraction covers both; the guard holds every bands case to nq >= 1
_DROPPED = {"chain_f32_kernel": (1, 2, 4, 5), "chain_marker_kernel": (1, 2, 3, 4), "time_f32_kernel": (1, 2), "iir_f64_kernel": (0,),
            "filter_q7_kernel": (1,), "fold_mag_f32_kernel": (0,), "hist_f32_kernel": (0,), "mask_f32_kernel": (1, 2),
            "bands_f32_kernel": (1,)}
_ONE_ROUND_AT = {"chain_f32_kernel": 5, "chain_marker_kernel": 4}
EXEMPT = {"one round": "B <= 512 rows of <= 128 KiB: 64 MiB",
          "sa_spin_kernel": "waits on the clock, reads and writes no memory"}
# forms of one instantiation that the launcher chooses at run time, each of which a case must take
RUNTIME_FORMS = {"hist_f32_kernel": ("one slice", "sliced")}


def address_form(key):
    """A kernel key without the template arguments that do not enter an address; None for a key of EXEMPT."""
    stem = re.match(r"\w+", key).group(0)
    if stem == "sa_spin_kernel":
        return None
    args = key[len(stem) + 1:-1].split(", ") if "<" in key else []
    if stem in _ONE_ROUND_AT and args[_ONE_ROUND_AT[stem]] == "true":
        return None
    kept = [a for i, a in enumerate(args) if i not in _DROPPED.get(stem, ())]
    return stem + (f"<{', '.join(kept)}>" if kept else "")


def required_forms(built):
    """The address forms of a set of built kernel keys, a kernel with run-time forms once per form."""
    out = set()
    for f in filter(None, map(address_form, built)):
        out |= {f"{f}: {r}" for r in RUNTIME_FORMS[f]} if f in RUNTIME_FORMS else {f}
    return out


def launched_forms(case):
    """The address forms a case launches."""
    out = set()
    for k in kernels(case):
        f = address_form(k)
        if f == "hist_f32_kernel":
            f += ": sliced" if "hist_zero_kernel" in kernels(case) else ": one slice"
        out.add(f)
    return out


# --------------------------------------------------------------------------------------------------------- the compare
def as_rows(torch, t, rows):
    """A contiguous tensor as [rows, words] int32: what the comparison looks at is bits."""
    if t.dtype == torch.complex64:
        t = torch.view_as_real(t)
    return t.reshape(rows, -1).view(torch.int32)


def tiled_mismatch(torch, out, ref):
    """None where every row r of `out` [R, words] equals row r mod P of `ref` [P, words] -- each whole period torch.equal to
    the reference, the tail to the reference's head -- else the first period that differs with its first differing rows.
    One period at a time: nothing of the size of `out` is made."""
    P = ref.shape[0]
    assert out.dim() == 2 and ref.dim() == 2 and out.shape[1] == ref.shape[1] and out.dtype == ref.dtype and P > 0
    for s in range(0, out.shape[0], P):
        n = min(P, out.shape[0] - s)
        if not torch.equal(out[s:s + n], ref[:n]):
            bad = torch.nonzero((out[s:s + n] != ref[:n]).any(dim=1)).flatten()
            return f"rows {[s + int(i) for i in bad[:5]]} ... ({bad.numel()} of the {n} rows from {s} on) differ from row mod {P}"
    return None


def vacuous(torch, ref, floating):
    """None where the reference rows [P, words] int32 are non-zero, pairwise different and (`floating`: the float32 view)
    finite, else what is wrong.  Rows with different 64-bit weighted sums are different rows."""
    if not bool((ref != 0).any(dim=1).all()):
        return "a reference row is all zero"
    if floating is not None and not bool(torch.isfinite(floating).all()):
        return "a reference row is not finite"
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    w = (torch.randint(1, 1 << 30, (ref.shape[1],), generator=g, dtype=torch.int64) | 1).to(ref.device)
    sums = (ref.to(torch.int64) * w).sum(dim=1)
    if torch.unique(sums).numel() != ref.shape[0]:
        return "two reference rows may be equal"
    return None
