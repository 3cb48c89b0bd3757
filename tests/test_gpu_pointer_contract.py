"""GPU: the pointer contract of the process and filter calls (include/specan.h, "pointer contract") at the eight entry
points themselves and through SpectrumChain, and every refusal of the one argument check (csrc/sa_pointers.cpp) at the eleven
data-plane entry points of include/specan.h and include/specan_ext.h.

tests/test_pointer_contract_cpu.py pins the rule (alignment, byte counts, the interval test) without a GPU.  Here: a refused
call launches nothing and leaves no trace on the handle; buffers that touch and row slices of the half layouts, which the
contract accepts, give the bits of the plain call.  A misaligned or overlapping pair of pointers is only ever passed to a
call that must refuse it, and every such pointer lies inside one allocation of the test."""
import functools

import numpy as np
import pytest

from conftest import N
from gpu_support import ch, synth, to_device, torch_mod  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SA_OK, SA_EINVAL = 0, -1
B = 5
HOP = 4104
CANARY = 0x5A
PAD = 4096
IN_FRAME = {"f32": 65536, "i16": 32768, "p12": 24576}
FLOAT_KINDS = {0: (65536, 16), 1: (8193 * 4, 4), 2: (8193 * 8, 8), 3: (65536, 16), 4: (16, 16)}      # kind: (row bytes, alignment)
Q15_KINDS = {0: (65536, 16), 1: (65536, 16), 2: (16, 16), 0x14: (8192, 16)}                           # 0x14: the trace, W = 16
# entry point -> (input form, takes scale, takes out_kind, {kind: (row bytes, alignment of out)}, takes a hop word)
ENTRIES = {
    "sa_process_f32": ("f32", False, True, FLOAT_KINDS, False),
    "sa_process_f32_i16": ("i16", True, True, FLOAT_KINDS, False),
    "sa_process_f32_p12": ("p12", True, True, FLOAT_KINDS, False),
    "sa_process_q15": ("i16", False, False, {0: (65536, 16)}, False),
    "sa_process_q15_out": ("i16", False, True, Q15_KINDS, True),
    "sa_process_q15_p12": ("p12", False, True, Q15_KINDS, True),
    "sa_filter_q15": ("i16", False, False, {0: (32768, 16)}, False),
    "sa_filter_q15_p12": ("p12", False, False, {0: (32768, 16)}, False),
}


@functools.lru_cache(maxsize=None)
def host_inputs():
    """One read-only batch for every test: 7 frames of 12-bit samples as int16 and packed, and 7 float frames."""
    from fpga_real_time_fft_analyzer_amd.ingest import pack12
    xi = np.random.default_rng(4242).integers(-2048, 2048, (7, N)).astype(np.int16)
    forms = {"i16": xi, "p12": pack12(xi), "f32": synth(7, 99)}
    for a in forms.values():
        a.setflags(write=False)
    return forms


def c_call(ch, name, in_ptr, out_ptr, batch, word=0):
    """The C entry point `name` on raw addresses; returns (code, sa_last_error)."""
    import torch
    _, takes_scale, takes_kind, _, _ = ENTRIES[name]
    args = (ch._h, in_ptr) + ((1.0 / 2048.0,) if takes_scale else ()) + (out_ptr, batch) + ((word,) if takes_kind else ())
    rc = getattr(ch._lib, name)(*args, torch.cuda.current_stream().cuda_stream)
    return rc, ch._lib.sa_last_error(ch._h).decode()


def in_bytes(form, hop, batch):
    if not hop:
        return batch * IN_FRAME[form]
    return ((batch - 1) * hop + N) * (3 if form == "p12" else 4) // 2


def configurations(name):
    """(filter byte, precision): one mode that stages through a workspace (0x00: the Q15 cascade; with 'f64' the float64
    cascade) and one that does not (0xB1)."""
    return ((0x00, "f32"), (0xB1, "f32"), (0x00, "f64")) if name.startswith("sa_process_f32") else ((0x00, "f32"), (0xB1, "f32"))


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refused_calls_launch_nothing_and_leave_no_trace(ch, torch_mod, name):
    """A misaligned `in`, a misaligned `out` and overlapping pairs at every kind of the entry point (and with a hop where it
    takes one): SA_EINVAL, the message names the entry point and the pointer, `out` -- a slice of a canary-filled tensor --
    is untouched, the profiling ring has no new entry, and the good call that follows gives the bits of the one made before."""
    torch = torch_mod
    form, _, _, kinds, hop_word = ENTRIES[name]
    d_in = to_device(torch, host_inputs()[form][:B])
    assert d_in.data_ptr() % 16 == 0
    misalign_in = {"f32": 4, "i16": 2, "p12": 1}[form]                 # one element into the buffer
    for cmd, precision in configurations(name):
        ch.set_filter_mode(cmd)
        ch.set_precision(precision)
        for kind, (row, align) in kinds.items():
            for hop in (0, HOP) if hop_word else (0,):
                word = kind | (hop // 8) << 8
                tag = (name, hex(cmd), precision, hex(word))
                n_in, n_out = in_bytes(form, hop, B), B * row
                good = torch.zeros(n_out, dtype=torch.uint8, device="cuda")
                assert good.data_ptr() % 16 == 0
                assert c_call(ch, name, d_in.data_ptr(), good.data_ptr(), B, word)[0] == SA_OK, tag
                ref = good.clone()
                assert ref.any(), tag
                ch.set_profiling(4)
                assert c_call(ch, name, d_in.data_ptr(), good.data_ptr(), B, word)[0] == SA_OK, tag
                assert len(ch.profile_read(4)) == 1
                # every address below lies inside `raw`, which is large enough for both ranges of any of the calls
                raw = torch.full((PAD + n_in + n_out + 16 + PAD,), CANARY, dtype=torch.uint8, device="cuda")
                out = raw.data_ptr() + PAD
                assert out % 16 == 0
                # the rules that were there before the contract keep their words
                in_words = "packed input" if form == "p12" else "sample stream" if hop else "`in` must be 16-byte aligned"
                out_words = "output must be 16-byte aligned" if row == 16 or kind == 0x14 else f"`out` must be {align}-byte aligned"
                refusals = (
                    (in_words, d_in.data_ptr() + misalign_in, out, B - 1),     # a misaligned `in` (one frame fewer: inside d_in)
                    (out_words, d_in.data_ptr(), out + align // 2, B),         # a misaligned `out`
                    ("overlap", out, out, B),                                  # out == in
                    ("overlap", out + 16, out, B),                             # `in` starts inside `out`
                    ("overlap", out, out + n_in - 16, B),                      # `out` starts inside `in`
                )
                for what, a_in, a_out, batch in refusals:
                    rc, msg = c_call(ch, name, a_in, a_out, batch, word)
                    assert rc == SA_EINVAL, tag + (what,)
                    assert msg.startswith(name + ":") and what in msg, tag + (what, msg)
                torch.cuda.synchronize()
                assert (raw == CANARY).all().item(), tag                                  # nothing was launched
                assert len(ch.profile_read(4)) == 1, tag                                  # no refused call was timed
                good.zero_()
                assert c_call(ch, name, d_in.data_ptr(), good.data_ptr(), B, word)[0] == SA_OK, tag
                assert len(ch.profile_read(4)) == 2, tag
                ch.set_profiling(0)
                assert torch.equal(good, ref), tag


@pytest.mark.parametrize("name", ["sa_process_f32", "sa_process_q15_out", "sa_filter_q15_p12"])
def test_refused_calls_in_overlap_mode_take_no_slot(ch, torch_mod, name):
    """Depth 2: a refused call between two good ones; after flush() both results are those of ordered mode."""
    torch = torch_mod
    form, _, _, kinds, _ = ENTRIES[name]
    row, _ = kinds[0]
    xs = [to_device(torch, host_inputs()[form][a:a + 3]) for a in (0, 3)]
    ch.set_filter_mode(0x00)
    ch.reserve(4)
    refs = []
    for x in xs:
        o = torch.zeros(3 * row, dtype=torch.uint8, device="cuda")
        assert c_call(ch, name, x.data_ptr(), o.data_ptr(), 3)[0] == SA_OK
        refs.append(o)
    torch.cuda.synchronize()
    assert refs[0].any() and not torch.equal(refs[0], refs[1])
    ch.set_overlap(2)
    outs = [torch.zeros(3 * row, dtype=torch.uint8, device="cuda") for _ in range(4)]
    canary = torch.full((3 * row + 16,), CANARY, dtype=torch.uint8, device="cuda")
    for k, o in enumerate(outs):
        assert c_call(ch, name, xs[k % 2].data_ptr(), o.data_ptr(), 3)[0] == SA_OK
        rc, msg = c_call(ch, name, xs[k % 2].data_ptr(), canary.data_ptr() + 8, 3)               # misaligned `out`
        assert rc == SA_EINVAL and msg.startswith(name + ":")
        rc, msg = c_call(ch, name, o.data_ptr(), o.data_ptr(), 3)                                # out == in
        assert rc == SA_EINVAL and "overlap" in msg
    ch.flush()
    torch.cuda.synchronize()
    ch.set_overlap(1)
    for k, o in enumerate(outs):
        assert torch.equal(o, refs[k % 2]), k
    assert (canary == CANARY).all().item()


# (entry point, kind word, hop): the float chain's mag_full, process_q15's wire frames, a hop stream
TOUCHING = (("sa_process_f32", 0, 0), ("sa_process_q15", 0, 0), ("sa_process_q15_out", 0 | (HOP // 8) << 8, HOP))


@pytest.mark.parametrize("cmd", [0x00, 0xB1])
@pytest.mark.parametrize("name,word,hop", TOUCHING)
def test_touching_buffers_are_accepted_and_correct(ch, torch_mod, name, word, hop, cmd):
    """`in` and `out` carved back to back from one allocation, in both orders: the result of the call on separate tensors,
    and the input bytes unchanged."""
    torch = torch_mod
    form, _, _, kinds, _ = ENTRIES[name]
    batch = 3
    n_in, n_out = in_bytes(form, hop, batch), batch * kinds[0][0]
    assert n_in % 16 == 0 and n_out % 16 == 0
    x = to_device(torch, host_inputs()[form][:batch]).view(torch.uint8).reshape(-1)[:n_in].clone()
    ch.set_filter_mode(cmd)
    ref = torch.zeros(n_out, dtype=torch.uint8, device="cuda")
    assert c_call(ch, name, x.data_ptr(), ref.data_ptr(), batch, word)[0] == SA_OK
    assert ref.any()
    for in_first in (True, False):
        one = torch.full((n_in + n_out,), CANARY, dtype=torch.uint8, device="cuda")
        a_in, a_out = (0, n_in) if in_first else (n_out, 0)
        one[a_in:a_in + n_in] = x
        p_in, p_out = one.data_ptr() + a_in, one.data_ptr() + a_out
        assert p_in % 16 == 0 and p_out % 16 == 0 and (p_out == p_in + n_in if in_first else p_in == p_out + n_out)
        rc, msg = c_call(ch, name, p_in, p_out, batch, word)
        assert rc == SA_OK, (in_first, msg)
        torch.cuda.synchronize()
        assert torch.equal(one[a_out:a_out + n_out], ref), in_first
        assert torch.equal(one[a_in:a_in + n_in], x), in_first


@pytest.mark.parametrize("form", ["f32", "i16"])
@pytest.mark.parametrize("cmd", [0xB1, 0x00])                              # the bypass kernel, the cascade kernel
@pytest.mark.parametrize("out_kind", ["mag_half", "spec_half"])
def test_row_slices_of_the_half_layouts(ch, torch_mod, out_kind, cmd, form):
    """process_f32(x[a:a+3], out=big[a:a+3]) for a = 1, 2, 3: rows of 8193 elements put the slice 4, 8 or 12 bytes (spec_half:
    8, 0, 8) off a 16-byte boundary.  The slice holds the rows of the whole-tensor call bit for bit; the rows before and
    behind it are still canary."""
    torch = torch_mod
    x = to_device(torch, host_inputs()[form])
    ch.set_filter_mode(cmd)
    whole = ch.process_f32(x, out_kind=out_kind).clone()
    assert whole.shape == (7, 8193) and whole.data_ptr() % 16 == 0
    words = whole.element_size() // 4
    canary = 0x7FC0BEEF                                                    # a NaN pattern
    residues = []
    for a in (1, 2, 3):
        bits = torch.full((7, 8193 * words), canary, dtype=torch.int32, device="cuda")
        big = bits.view(whole.dtype)
        assert big.shape == whole.shape and big.data_ptr() % 16 == 0
        out = big[a:a + 3]
        residues.append(out.data_ptr() % 16)
        assert out.is_contiguous() and out.data_ptr() % 16 == a * 8193 * whole.element_size() % 16
        got = ch.process_f32(x[a:a + 3], out=out, out_kind=out_kind)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(bits[a:a + 3], whole.view(torch.int32).view(7, -1)[a:a + 3]), (a, out_kind)
        assert (bits[:a] == canary).all().item() and (bits[a + 3:] == canary).all().item(), (a, out_kind)
    assert residues == ([4, 8, 12] if out_kind == "mag_half" else [8, 0, 8])
    assert torch.isfinite(whole.view(torch.float32)).all().item() and whole.view(torch.float32).any().item()


def test_wrapper_surfaces_the_refusals(ch, torch_mod):
    """SpectrumChain needs no check of its own: a contiguous view one element into a buffer and `out=x` come back as
    SpecanError with code SA_EINVAL, and the handle goes on as before."""
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    torch = torch_mod
    xf = to_device(torch, host_inputs()["f32"][:2])
    xi = to_device(torch, host_inputs()["i16"][:2])
    ch.set_filter_mode(0x00)
    ref_f, ref_q, ref_t = ch.process_f32(xf).clone(), ch.process_q15(xi).clone(), ch.filter_q15(xi).clone()

    def refused(what, fn, *a, **kw):
        with pytest.raises(SpecanError) as e:
            fn(*a, **kw)
        assert e.value.code == SA_EINVAL and what in str(e.value), (what, str(e.value))

    off_f = torch.zeros(2 * N + 1, dtype=torch.float32, device="cuda")[1:].view(2, N)
    off_i = torch.zeros(2 * N + 1, dtype=torch.int16, device="cuda")[1:].view(2, N)
    off_f.copy_(xf)
    off_i.copy_(xi)
    assert off_f.is_contiguous() and off_f.data_ptr() % 16 == 4 and off_i.is_contiguous() and off_i.data_ptr() % 16 == 2
    refused("sa_process_f32: `in`", ch.process_f32, off_f)
    refused("sa_process_f32_i16: `in`", ch.process_f32, off_i)
    refused("sa_process_q15: `in`", ch.process_q15, off_i)
    refused("sa_process_q15_out: `in`", ch.process_q15, off_i, out_kind="mag")
    refused("sa_filter_q15: `in`", ch.filter_q15, off_i)
    refused("sa_process_f32: `out`", ch.process_f32, xf, out=off_f)
    refused("sa_filter_q15: `out`", ch.filter_q15, xi, out=off_i)
    keep_f, keep_i = xf.clone(), xi.clone()
    refused("overlap", ch.process_f32, xf, out=xf)                         # mag_full in place
    refused("overlap", ch.process_f32, xf, out=xf, out_kind="time")
    refused("overlap", ch.filter_q15, xi, out=xi)
    torch.cuda.synchronize()
    assert torch.equal(xf, keep_f) and torch.equal(xi, keep_i)
    assert torch.equal(ch.process_f32(xf), ref_f) and torch.equal(ch.process_q15(xi), ref_q)
    assert torch.equal(ch.filter_q15(xi), ref_t)


# ---- every entry point is wired to the one argument check (sa_check_call, csrc/sa_pointers.cpp)
SA_ESHAPE = -2
AVG, TRACE = 0x80 | 2 << 3 | 4, 0x10 | 4                    # SA_Q15_TRACE_AVG_KIND(4, 2): A = 4; SA_Q15_TRACE_KIND(4)
HOPW = (4096 // 8) << 8                                     # the hop field of SA_Q15_HOP_KIND(kind, 4096)
# entry point -> (input form, (bytes read, bytes written) of the plain call on 4 frames -- the ext calls: groups of A = 4)
WIRED = {
    "sa_process_f32": ("f32", (262144, 262144)), "sa_process_f32_i16": ("i16", (131072, 262144)),
    "sa_process_f32_p12": ("p12", (98304, 262144)), "sa_process_q15": ("i16", (131072, 262144)),
    "sa_process_q15_out": ("i16", (131072, 262144)), "sa_process_q15_p12": ("p12", (98304, 262144)),
    "sa_filter_q15": ("i16", (131072, 131072)), "sa_filter_q15_p12": ("p12", (98304, 131072)),
    "sa_spectra_q15": ("i16", (131072, 131072)), "sa_spectra_q15_p12": ("p12", (98304, 131072)),
    "sa_fold_iq_q15": ("iq", (262144, 131072)),
}


def wired_refusals(name, IN, OUT):
    """(words of sa_last_error behind the entry point's name, code, arguments that differ from the good call) for each rule
    that `name` can reach through its C argument list with addresses inside one allocation: all but the workspace rule, whose
    batch no allocation holds (tests/cpp/test_sa_call_check.cpp has it).  The words are written out here."""
    form, (n_in, n_out) = WIRED[name]
    in_words = "packed input must be 16-byte aligned" if form == "p12" else "`in` must be 16-byte aligned"
    off = {"f32": 4, "i16": 2, "p12": 1, "iq": 4}[form]
    r = [("negative batch", SA_ESHAPE, dict(batch=-1)),
         ("NULL tensor", SA_EINVAL, dict(a_in=0)),
         ("NULL tensor", SA_EINVAL, dict(a_out=0)),
         (in_words, SA_EINVAL, dict(a_in=IN + off)),
         ("`out` must be 16-byte aligned", SA_EINVAL, dict(a_out=OUT + 8)),
         (f"`in` ({n_in} bytes read) and `out` ({n_out} bytes written) overlap", SA_EINVAL, dict(a_out=IN))]
    if name.startswith("sa_process_f32"):
        r += [("bad out_kind", SA_EINVAL, dict(word=5)),
              ("bad out_kind", SA_EINVAL, dict(word=5, batch=0)),
              ("`out` must be 4-byte aligned", SA_EINVAL, dict(word=1, a_out=OUT + 2)),
              ("`out` must be 8-byte aligned", SA_EINVAL, dict(word=2, a_out=OUT + 4)),
              ("SA_OUT_MARKER output must be 16-byte aligned", SA_EINVAL, dict(word=4, a_out=OUT + 8)),
              ("SA_OUT_MARKER output must be 16-byte aligned", SA_EINVAL, dict(word=4, a_in=IN + off, a_out=OUT + 8)),
              (in_words, SA_EINVAL, dict(word=0, a_in=IN + off, a_out=OUT + 8))]
        if name != "sa_process_f32":
            r += [("scale is not finite", None, dict(scale=float("nan"))),           # the export has no scale: the code below
                  ("scale is not finite", None, dict(scale=float("inf"), batch=0)),
                  ("bad out_kind", SA_EINVAL, dict(word=5, scale=float("nan")))]
    if name in ("sa_process_q15_out", "sa_process_q15_p12"):
        stream = "packed input must be 16-byte aligned" if form == "p12" else "a sample stream (SA_Q15_HOP_KIND) must be 16-byte aligned"
        r += [("bad out_kind: hop field above 2048 or bits 20..30 set", SA_EINVAL, dict(word=0 | 2049 << 8)),
              ("bad out_kind: hop field above 2048 or bits 20..30 set", SA_EINVAL, dict(word=3 | 1 << 20, batch=0)),
              ("bad out_kind", SA_EINVAL, dict(word=3)),
              ("bad out_kind", SA_EINVAL, dict(word=0x88, batch=0)),
              ("SA_Q15_TRACE_AVG_KIND: batch must be a multiple of the group size A", SA_ESHAPE, dict(word=AVG, batch=5)),
              ("SA_Q15_TRACE_AVG_KIND: batch must be a multiple of the group size A", SA_ESHAPE, dict(word=AVG | HOPW, batch=5, a_in=0)),
              (stream, SA_EINVAL, dict(word=0 | HOPW, a_in=IN + off)),
              ("SA_Q15_OUT_MARKER output must be 16-byte aligned", SA_EINVAL, dict(word=2, a_out=OUT + 8)),
              ("SA_Q15_TRACE_KIND output must be 16-byte aligned", SA_EINVAL, dict(word=TRACE, a_out=OUT + 8)),
              ("SA_Q15_TRACE_AVG_KIND output must be 16-byte aligned", SA_EINVAL, dict(word=AVG | HOPW, a_out=OUT + 8)),
              ("SA_Q15_OUT_MARKER output must be 16-byte aligned", SA_EINVAL, dict(word=2, a_in=IN + off, a_out=OUT + 8)),
              (in_words, SA_EINVAL, dict(word=1, a_in=IN + off, a_out=OUT + 8))]
    if name.startswith("sa_spectra") or name == "sa_fold_iq_q15":
        r += [("log2a must be 1..7 (groups of A = 2..128 frames)", SA_EINVAL, dict(log2a=0)),
              ("log2a must be 1..7 (groups of A = 2..128 frames)", SA_EINVAL, dict(log2a=8, batch=0)),
              ("negative batch", SA_ESHAPE, dict(log2a=0, batch=-1)),
              ("batch must be a multiple of the group size A", SA_ESHAPE, dict(batch=5)),
              ("batch must be a multiple of the group size A", SA_ESHAPE, dict(batch=5, a_in=0, a_out=0))]
    if name.startswith("sa_spectra"):                       # the C argument list of the fold has no hop to refuse
        stream = "packed input must be 16-byte aligned" if form == "p12" else "a sample stream must be 16-byte aligned"
        r += [("hop must be 0 or a multiple of 8 in 8..16384", SA_EINVAL, dict(hop=4)),
              ("hop must be 0 or a multiple of 8 in 8..16384", SA_EINVAL, dict(hop=16392, batch=0)),
              (stream, SA_EINVAL, dict(hop=4096, a_in=IN + off))]
    return r


def test_every_entry_point_runs_the_one_check(ch, torch_mod):
    """For each of the eleven C entry points and each rule it can reach: the code is the one the handle-free export gives for
    the same arguments, sa_last_error is the entry point's name and the rule's words, nothing is written and nothing timed.
    Every address lies inside one canary-filled allocation that holds both ranges of any of these calls; a misaligned or
    overlapping pair only ever goes to a call that must refuse it.  Before that, the one accepted call whose host path is
    new: the fold alone gives the bits of spectra_q15 on the same frames."""
    from fpga_real_time_fft_analyzer_amd import abi
    torch = torch_mod
    L = ch._lib
    stream = torch.cuda.current_stream().cuda_stream
    ch.set_filter_mode(0x00)
    x = to_device(torch, host_inputs()["i16"][:4])
    want = ch.spectra_q15(x, 2)
    got = ch.fold_iq_q15(ch.process_q15(x, out_kind="iq"), 2)
    torch.cuda.synchronize()
    assert got.shape == (2, N, 2) and torch.equal(got.view(torch.int32), want.view(torch.int32)) and want.any().item()

    half = 1 << 20
    raw = torch.full((PAD + 2 * half,), CANARY, dtype=torch.uint8, device="cuda")
    IN = raw.data_ptr() + PAD
    OUT = IN + half
    assert IN % 16 == 0 and 5 * 65544 + 16 < half - PAD
    ch.set_profiling(8)
    timed = len(ch.profile_read(8))
    assert list(WIRED) == list(abi.SA_ENTRIES) + list(abi.SA_EXT_ENTRIES)
    for entry, name in enumerate(WIRED):
        ext = entry >= 8
        fn = getattr(L, name)
        for words, code, change in wired_refusals(name, IN, OUT):
            a = dict(a_in=IN, a_out=OUT, batch=4, word=0, log2a=2, hop=0, scale=1.0 / 2048.0)
            a.update(change)
            tag = (name, words, change)
            if ext:
                exported = L.sa_ext_check_pointers(entry - 8, a["log2a"], a["hop"], a["a_in"], a["a_out"], a["batch"])
                tail = (a["log2a"],) + ((a["hop"],) if name != "sa_fold_iq_q15" else ())
            else:
                exported = L.sa_debug_check_pointers(entry, a["word"], a["a_in"], a["a_out"], a["batch"])
                tail = (a["word"],) if ENTRIES[name][2] else ()
            if code is None:                                # a scale that is not finite: the export has no scale to refuse
                assert exported == SA_OK, tag
                exported = SA_EINVAL
            else:
                assert exported == code, tag                # what this file expects of the export, written out
            head = (a["a_in"],) + ((a["scale"],) if not ext and ENTRIES[name][1] else ()) + (a["a_out"], a["batch"])
            rc = fn(ch._h, *head, *tail, stream)
            assert rc == exported, tag + (rc,)
            assert L.sa_last_error(ch._h).decode() == name + ": " + words, tag
            assert fn(None, *head, *tail, stream) == SA_EINVAL, tag                       # no handle: no message either
    torch.cuda.synchronize()
    assert (raw == CANARY).all().item()                     # nothing was launched
    assert len(ch.profile_read(8)) == timed                 # no refused call was timed
    ch.set_profiling(0)
    assert torch.equal(ch.spectra_q15(x, 2), want)          # the handle goes on
