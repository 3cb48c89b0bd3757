"""CPU: the guard of tests/offset_cases.py, the table behind tests/test_gpu_offsets.py.  It holds every case's batch and period
to the rules from the outside (the last row of the deciding tensor starts at or beyond 2^32, the row before the extra rows
below it; the period is a multiple of the group, above 512 and no divisor of a power of two), the union of what the cases
launch to the symbol tables of every built library -- libspecan_hip.so and each row of abi.LIBRARIES --, and the cases to the
entry points and chain tables of abi.py and chain.py: a kernel, an entry point, a library, an input form or an output kind
added later fails here until a case covers it.  The
comparison the GPU test relies on is tested here too, on CPU tensors at a scaled-down modulus."""
import os
import re

import pytest

import drawn_cases as dc
import offset_cases as oc
from fpga_real_time_fft_analyzer_amd import abi, chain, reductions
from kernel_inventory import inventory
from native import CSRC
from offset_cases import CASES, TWO31, TWO32

# a case removed (or added) on purpose changes this number with it: the 60 of the chains, the fold, the histogram in two
# forms, and magnitudes and both fields of records on each of the seven libraries that read records
N_CASES = 60 + 1 + 2 + 3 * len(dc.HAS_FIELD)


def _figures(case):
    """name -> (bytes per row, rows, bytes, start of the last row)"""
    return {k: (rb, rows, rb * rows, oc.last_row_start(rb, rows)) for k, (rb, rows) in oc.tensors(case).items()}


def test_batches_and_periods_obey_the_rules():
    """Every case: B a multiple of A; P a multiple of A, above 512, and for no tensor of the case is 2^31 or 2^32 a multiple
    of P / A rows' bytes; the last row of the deciding tensor -- the smallest spectrum-sized one -- starts at or beyond 2^32,
    and the row before the at most three extra rows starts below it.  Prints every tensor that passes 2^31 or 2^32."""
    assert len(CASES) == N_CASES == 84
    assert 0 <= oc.EXTRA <= 3
    for c in CASES:
        assert c.B % c.A == 0 and c.P % c.A == 0 and c.P > 512, c
        fig = _figures(c)
        for name, (rb, rows, total, last) in fig.items():
            per = c.P // c.A * rb
            assert TWO31 % per and TWO32 % per, (c.id, name, per)
        name, rb = oc.deciding_tensor(c)
        assert rb == min(v[0] for v in fig.values() if v[0] >= oc.SPECTRUM_BYTES), (c.id, name)
        rows = fig[name][1]
        assert oc.last_row_start(rb, rows) >= TWO32, (c.id, name, rows)
        assert oc.last_row_start(rb, rows - oc.EXTRA - 1) < TWO32, (c.id, name, rows, "B is larger than the rule allows")
        assert oc.last_row_start(rb, rows - oc.EXTRA) >= TWO32, (c.id, name, rows)
        past = {k: ("2^32" if v[3] >= TWO32 else "2^31") for k, v in fig.items() if v[3] >= TWO31}
        print(f"{c.id}: A {c.A} P {c.P} B {c.B} decided by {name} ({rb} B/row); "
              + ", ".join(f"{k} {v[2]} B last row past {past.get(k, 'neither')}" for k, v in fig.items()))
    # the figures the rule gives: float32 frames, int16 frames, packed frames, rows of 128 KiB records
    by = oc.BY_ID
    assert by["process_f32-f32-mag_full-butter12"].B == 65536 + 1 + oc.EXTRA
    assert by["process_q15-i16-iq-b1_rtl"].B == 131072 + 1 + oc.EXTRA
    assert by["process_q15-p12-iq-b1_rtl"].B == 174763 + 1 + oc.EXTRA
    assert by["find_peaks-rec-field=peak"].B == 32768 + 1 + oc.EXTRA
    # the handle-free calls: 65 539 rows of magnitudes, 32 771 rows of records -- but cfar, whose spectrum-sized output decides
    assert {c.B // c.A for c in CASES if c.form == "mag"} == {65536 + 1 + oc.EXTRA, 32768 + 1 + oc.EXTRA}          # A = 1, A = 2
    assert {(c.call == "cfar", c.B) for c in CASES if c.form == "rec"} == {(False, 32768 + 1 + oc.EXTRA), (True, 65536 + 1 + oc.EXTRA)}
    assert {c.id for c in CASES if c.call in oc.LIBRARY and oc.deciding_tensor(c)[0] == "out"} == {
        "cfar-rec-field=peak", "cfar-rec-field=power"}
    assert all(_figures(c)["in"][2] > 2 * TWO32 and _figures(c)["out"][3] >= TWO32 for c in CASES if c.call == "cfar" and c.form == "rec")
    assert _figures(by["cfar-mag-field=all"])["out"][3] >= TWO32
    assert {c.P for c in CASES} == {1027, 514} and oc.period(1) == 1027 and oc.period(2) == 2 * 257
    # the reduced outputs never reach 2^31; their inputs pass 2^32.  Of the handle-free calls all but the fold and cfar
    # reduce, and every tensor beside the input is held so: power and cross, stats, a threshold per row, the count
    reduced = set(oc.LIBRARY) - {"fold_mag_f32", "cfar"}
    assert len(reduced) == len(abi.LIBRARIES) - 2
    for c in CASES:
        if c.kind == "marker" or c.call in reduced:
            fig = _figures(c)
            assert fig["in"][3] >= TWO32 and all(v[2] < TWO31 for k, v in fig.items() if k != "in" and not k.startswith("ws_")), c.id
    # every tensor of a call that grows with the batch is there, by the names of drawn_cases.outputs
    names = {c.call: set(oc.tensors(c)) - {"in"} for c in CASES if c.call in oc.LIBRARY and c.params.get("group", 1) is not None}
    assert names == {"fold_mag_f32": {"out"}, "find_peaks": {"out", "count"}, "order_stats": {"out"}, "level_hist": {"out"},
                     "band_power": {"power", "cross"}, "mask_test": {"out"}, "harmonics": {"out"},
                     "find_signals": {"out", "stats", "threshold"}, "cfar": {"out"}}, names
    # the workspaces that pass 2^32: the grouped trace's partial records at 128 KiB per frame, the IQ frames of spectra_q15,
    # the cascade's int16 frames and the float64-state path's float32 frames
    reached = {name for c in CASES for name, v in _figures(c).items() if name.startswith("ws_") and v[3] >= TWO32}
    assert reached == {"ws_trace", "ws_iq", "ws_q15", "ws_f64"}, reached
    c = by["traces_q15-i16-2x2-b1_rtl"]
    assert oc.tensors(c)["ws_trace"][0] == c.A * 128 * 1024


def test_byte_counts_that_the_python_layer_does_not_hold():
    """The partial record of the grouped trace is kSaTraceRawBytes of csrc/sa_common.hpp, and the slice rule mirrors the
    constants of csrc/sa_hist.hpp; the merged histogram runs in unequal row slices, the grouped one in one."""
    text = open(os.path.join(CSRC, "sa_common.hpp")).read()
    assert int(re.search(r"constexpr int kSaTraceRawBytes = (\d+);", text).group(1)) == oc.TRACE_RAW_RECORD_BYTES
    text = open(os.path.join(CSRC, "sa_hist.hpp")).read()
    m = re.search(r"kHistOwnersFew = (\d+), kHistOwnersAim = (\d+), kHistSliceRowsMin = (\d+);", text)
    assert tuple(map(int, m.groups())) == (256, 512, 32) and "kHistTile = 256;" in text
    merged, grouped = oc.BY_ID["level_hist-mag-group=all"], oc.BY_ID["level_hist-mag-group=2"]
    s = dc.hist_slices(merged.B, merged.B, merged.params["bucket"])
    assert s == 8 and merged.B % 2 == 1 and merged.B % s, (s, merged.B)               # slices of unequal length
    assert dc.hist_slices(grouped.B, 2, grouped.params["bucket"]) == 1
    assert dc.hist_slices(merged.P, merged.P, merged.params["bucket"]) > 1           # the period call is sliced as well
    assert chain.frames.HIST_GROUP_MAX >= merged.B


def test_cases_launch_every_address_form_of_the_built_libraries(hip_lib_built):
    """The kernel instantiations of every built library, without the template arguments that enter no address
    (offset_cases._DROPPED says why) and without the exempt ones, against the union of what the cases launch: equal.  What
    a case claims to launch exists in the libraries.  A dummy kernel key fails it."""
    built = set()
    for path in [abi.LIB_PATH] + [os.path.join(os.path.dirname(abi.LIB_PATH), name) for name, _ in abi.LIBRARIES.values()]:
        built |= inventory(path)
    exempt = {k for k in built if oc.address_form(k) is None}
    assert exempt and all("true" in k or k == "sa_spin_kernel" for k in exempt), sorted(exempt)
    print(f"exempt ({oc.EXEMPT}): {len(exempt)} instantiations")
    raw = {k for c in CASES for k in oc.kernels(c)}
    assert raw <= built, sorted(raw - built)
    need = oc.required_forms(built)
    have = set().union(*(oc.launched_forms(c) for c in CASES))
    assert have == need, ("no case launches", sorted(need - have), "launched but not built", sorted(have - need))
    assert oc.required_forms(built | {"dummy_kernel<short>"}) != have
    # the forms the table is meant to reach, counted
    count = lambda stem: sum(f.startswith(stem) for f in need)      # noqa: E731
    assert count("fft_q15_kernel<") == 25 and count("filter_q7_kernel<") == 4 and count("filter_w14_kernel<") == 4
    assert count("window_q15_kernel<") == 2 and count("iir_f64_kernel<") == 3 and count("chain_f32_kernel<") == 9
    assert count("chain_marker_kernel<") == 3 and count("time_f32_kernel<") == 3 and count("hist_f32_kernel") == 2
    # one form per field of each library that reads records (UP, LOW and CROSS dropped), and the summary of the mask test
    for x in dc.HAS_FIELD:
        assert count(f"{x}_f32_kernel<") == len(reductions.FIELDS) == 3, x
    assert count("mask_summary_kernel") == 1 and "mask_summary_kernel" in need
    # CROSS is dropped because a call with a fraction makes every access of one without: no bands case may have none
    bands = [c for c in CASES if c.call == "band_power"]
    assert bands and all(len(c.params["fracs"]) >= 1 for c in bands), [c.id for c in bands]
    print(f"{len(built)} instantiations, {len(need)} address forms, {len(CASES)} cases")


def test_cases_cover_the_entry_points_and_the_chain_tables():
    """Every C data-plane entry point, every (chain table, dtype, frames / stream) row of chain.py, both hops on both stream
    forms, and every output kind whose row is 32 KiB or more in a case where that output's last row starts at or beyond
    2^32.  The kinds of the grouped calls that differ in the group size A alone are one layout: they are held at A = 2, the
    smallest batch (at A = 128 the int16 input of such a case is 275 GB)."""
    entries = set(abi.SA_ENTRIES) | set(abi.SA_EXT_ENTRIES)
    assert len(entries) == 11
    for _, signatures in abi.LIBRARIES.values():                    # one data-plane entry point per handle-less library
        assert len(oc.data_plane(signatures)) == 1
        entries |= oc.data_plane(signatures)
    assert len(entries) == 11 + len(abi.LIBRARIES) == 20
    assert set(oc.LIBRARY.values()) == set(abi.LIBRARIES)
    assert {oc.entry_point(c) for c in CASES} == entries
    rows = set()
    for table in oc.CHAIN_TABLES:
        ch = getattr(chain, table)
        rows |= {(table, oc._torch_name(d), "frames") for d in ch.inputs} | {(table, oc._torch_name(d), "stream") for d in ch.streams}
    assert len(rows) == 22
    assert {oc.table_row(c) for c in CASES if oc.chain_table(c)} == rows
    assert {n for n in dir(chain) if n.endswith("_CHAIN")} == set(oc.CHAIN_TABLES)
    assert {(c.form, c.hop) for c in CASES if c.hop} == {(f, h) for f in ("i16_hop", "p12_hop") for h in oc.HOPS}

    def layout(table, kind):          # a kind of a grouped call without its group size
        return kind[0] if table == "Q15_TRACE_AVG_CHAIN" else "records" if table in ("Q15_SPECTRA_CHAIN", "Q15_FOLD_CHAIN") else kind

    need, have = set(), set()
    for c in CASES:
        table = oc.chain_table(c)
        if table and "out" in oc.tensors(c):
            rb, n = oc.tensors(c)["out"]
            if oc.last_row_start(rb, n) >= TWO32:
                have.add((table, layout(table, c.kind)))
    for table in oc.CHAIN_TABLES:
        ch = getattr(chain, table)
        for kind in ch.outputs:
            shape, dtype = chain.output_spec(ch, kind, ch.output(kind)[3])
            if oc._prod(shape[1:]) * oc.ITEMSIZE[oc._torch_name(dtype)] >= 32 * 1024:
                need.add((table, layout(table, kind)))
    assert need == {("FLOAT_CHAIN", "mag_full"), ("FLOAT_CHAIN", "mag_half"), ("FLOAT_CHAIN", "spec_half"), ("FLOAT_CHAIN", "time"),
                    ("Q15_CHAIN", "iq"), ("Q15_CHAIN", "mag"), ("Q15_TRACE_CHAIN", 2), ("Q15_TRACE_CHAIN", 4),
                    ("Q15_TRACE_AVG_CHAIN", 2), ("Q15_TRACE_AVG_CHAIN", 4), ("Q15_WINDOW_CHAIN", None),
                    ("Q15_SPECTRA_CHAIN", "records"), ("Q15_FOLD_CHAIN", "records")}, need
    assert need <= have, sorted(need - have, key=str)
    # the handle-free calls: three fields of every library that reads records, the fold, and the histogram in both forms
    assert {(c.call, c.params["field"]) for c in CASES if "field" in c.params} == {
        (dc.METHODS[x], f) for x in dc.HAS_FIELD for f in (None, "peak", "power")}
    assert set(reductions.FIELDS) == {None, "peak", "power"} and len(dc.HAS_FIELD) == 7
    assert {c.params["group"] for c in CASES if c.call == "level_hist"} == {2, None}
    # one cascade setup per kernel stem, and the float64-state path on every input type
    assert {c.setup for c in CASES if oc.chain_table(c) and oc.chain_table(c) != "FLOAT_CHAIN" and c.setup} == set(oc.Q15_CASCADES)
    assert {c.form for c in CASES if c.precision == "f64"} == {"f32", "i16", "p12"}


# ------------------------------------------------------------------------------------------------- the comparison helper
def test_the_comparison_sees_a_wrapped_offset():
    """tiled_mismatch on CPU tensors at a scaled-down modulus: 37 rows of 8 words, period 5, "2^32" at row 32.  A clean tiled
    output is accepted; rejected are rows from r0 on left at the sentinel (a kernel that stopped), rows from r0 on equal to
    rows r - r0 (a wrapped read), and one early row overwritten by a late row's value (a wrapped store)."""
    import torch
    P, R, r0 = 5, 37, 32
    g = torch.Generator()
    g.manual_seed(1)
    ref = torch.randint(-2 ** 31, 2 ** 31 - 1, (P, 8), generator=g, dtype=torch.int64).to(torch.int32)
    assert oc.vacuous(torch, ref, None) is None
    clean = torch.cat([ref] * (R // P + 1))[:R].clone()
    assert oc.tiled_mismatch(torch, clean, ref) is None
    stopped = clean.clone()
    stopped[r0:] = -1                                                    # 0xFF bytes
    assert "rows [32, 33, 34]" in oc.tiled_mismatch(torch, stopped, ref)
    wrapped_read = clean.clone()
    wrapped_read[r0:] = clean[:R - r0]                                   # row r holds what row r - r0 should
    assert r0 % P and "rows [32," in oc.tiled_mismatch(torch, wrapped_read, ref)
    wrapped_store = clean.clone()
    wrapped_store[R - 1 - r0] = clean[R - 1]                             # the store of row 36 landed on row 4
    assert "rows [4]" in oc.tiled_mismatch(torch, wrapped_store, ref)
    tail = clean.clone()
    tail[R - 1, 7] ^= 1                                                  # one bit of the last row
    assert "rows [36]" in oc.tiled_mismatch(torch, tail, ref)
    # a reference that could not tell: a zero row, two equal rows, a NaN
    z = ref.clone()
    z[2] = 0
    assert oc.vacuous(torch, z, None) == "a reference row is all zero"
    z = ref.clone()
    z[3] = z[1]
    assert oc.vacuous(torch, z, None) == "two reference rows may be equal"
    f = torch.ones((P, 8))
    f[4, 0] = float("nan")
    assert oc.vacuous(torch, ref, f) == "a reference row is not finite"
    # as_rows: complex and int16 outputs as int32 words
    assert oc.as_rows(torch, torch.zeros((3, 5), dtype=torch.complex64), 3).shape == (3, 10)
    assert oc.as_rows(torch, torch.zeros((3, 4, 2), dtype=torch.int16), 3).shape == (3, 4)
