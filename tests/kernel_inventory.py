"""Shared by tests/test_gpu_isolation.py (a plain module, like structured_cases.py): the kernel instantiations of the built
library, read from its symbol table, the names the isolation tests' variant tuples stand for, and the table that says of
every instantiation how the suite knows it does not read LDS words it did not write.

The compiler emits one host function `__device_stub__<kernel>` per kernel instantiation of a unit; the symbol table lists
them demangled.  The key used here is the kernel's name with its template arguments and without its argument list, the
anonymous namespace dropped: "fft_q15_kernel<short, false, 128>", "chain_f32_kernel<SaP12, 4, true, 0, false, false, float>",
"filter_w14_kernel<short, int>".

TABLE classifies every key as exactly one of
  "float:<group>"       poisoned by test_poisoned_lds_float_chain[<group>]: the group's variant set holds a tuple whose
                        launches (float_kernels) include the key;
  "q15:<case>"          poisoned by test_poisoned_lds_integer_chain[<case>], likewise (q15_kernels);
  "exempt: <why>"       uses no LDS at all -- proven by the inventory test from the compiler's resource remarks and the
                        unit's source (NO_LDS_UNITS), never taken on trust;
  "unreachable: <why>"  built, but no public call launches it: <why> names the dispatch line.
TABLE is built from the rules by which the launchers of csrc/ choose an instantiation (float_rows, q15_rows: each rule
names the dispatch line it mirrors) and reads nothing from the built library.  A kernel added to the library (or removed
from it) fails tests/test_gpu_isolation.py::test_kernel_inventory_is_classified without a GPU until a rule here covers it --
and a "float:" / "q15:" row holds only if that case's pinned variant set, which the GPU test asserts equal to what it
launched, contains the kernel."""
import os
import re

import native
from native import CSRC

STUB = "__device_stub__"


def key_of(function):
    """A demangled function, from its name on -> the key: name plus template arguments, the argument list dropped."""
    s = function.replace("(anonymous namespace)::", "")
    name = re.match(r"\w+", s).group(0)
    rest = s[len(name):]
    if not rest.startswith("<"):
        return name
    depth = 0
    for i, c in enumerate(rest):
        depth += (c == "<") - (c == ">")
        if depth == 0:
            return name + rest[:i + 1]
    raise ValueError(function)


def normalise(demangled):
    """A demangled stub symbol -> the key of its kernel."""
    return key_of(demangled.replace("(anonymous namespace)::", "").split(STUB, 1)[1])


def inventory(lib_path):
    """The keys of every kernel instantiation in the shared object, from its demangled symbol table (local symbols included)."""
    out = native.output_of([native.NM, "-C", lib_path], timeout=120)
    keys = [normalise(ln.split(None, 2)[2]) for ln in out.splitlines() if STUB in ln and len(ln.split(None, 2)) == 3]
    assert len(keys) == len(set(keys)), sorted(k for k in keys if keys.count(k) > 1)
    return set(keys)


# ---------------------------------------------------------------------------------------- what a variant tuple launches
CXX_IN = {"float32": "float", "int16": "short", "uint8": "SaP12"}                # torch dtype of x -> InT of the kernels
FLOAT_OUT = {"mag_full": 0, "mag_half": 1, "spec_half": 2}                       # SA_OUT_* of chain_f32_kernel's OUT


def _b(v):
    return "true" if v else "false"


def _chain_kernel(in_t, nsec, unit, wingen, one_round, kind):
    """One launch of chain_f32.hpp (launch_nsec / launch_spectrum); the kernels of int16 and packed samples carry the
    scale's type as a trailing pack argument."""
    t, pack = CXX_IN[in_t], "" if in_t == "float32" else ", float"
    if kind == "time":
        return f"time_f32_kernel<{t}, {nsec}, {_b(unit)}{pack}>"
    if kind == "marker":
        return f"chain_marker_kernel<{t}, {nsec}, {_b(unit)}, {_b(wingen)}, {_b(one_round)}{pack}>"
    return f"chain_f32_kernel<{t}, {nsec}, {_b(unit)}, {FLOAT_OUT[kind]}, {_b(wingen)}, {_b(one_round)}{pack}>"


def float_kernels(variant):
    """(InT, nsec, unit, wingen, one_round, out_kind, precision) of test_gpu_isolation._launched_f32 -> the keys of the
    launches of that process_f32 call, in order: one fused kernel, or iir_f64_kernel and (unless 'time') the bypassed
    chain on its float32 output."""
    in_t, nsec, unit, wingen, one_round, kind, precision = variant
    if precision == "f64":
        first = f"iir_f64_kernel<{nsec}, {CXX_IN[in_t]}>"
        return (first,) if kind == "time" else (first, _chain_kernel("float32", 0, 0, 0, one_round, kind))
    return (_chain_kernel(in_t, nsec, unit, wingen, one_round, kind),)


# input form -> the template arguments that name it: (InT,) in front, and behind the kernel's own arguments the `int` of the
# forms cut from one stream
Q15_FORM_SUFFIX = {"i16": (("short",), ()), "p12": (("SaP12",), ()), "i16_hop": (("short",), ("int",)),
                   "p12_hop": (("SaP12",), ("int",))}
# call -> (OUT of fft_q15_kernel, the fold launch behind it)
Q15_CALL = {"iq": (0, None), "mag": (1, None), "marker": (2, None), "trace": (16, None),
            "trace_avg": (128, "trace_fold_q15_kernel"), "spectra": (0, "spectra_fold_q15_kernel")}


def _tmpl(name, *args):
    return f"{name}<{', '.join(str(a) for a in args)}>"


def q15_kernels(cascade, form, call):
    """The keys of the launches of one Q15 call, in order (specan_abi.cpp, launch_q15).  `cascade`: None in filter mode
    0xB1, else the cascade kernel's stem and its own template arguments, those between InT and the hop --
    ("filter_q7", ("true",)), ("filter_q7", ("false",)) or ("filter_w14", ()); `form`: a key of Q15_FORM_SUFFIX; `call`:
    "filter" (filter_q15) or a key of Q15_CALL.  The input form names the kernel that reads the samples; an FFT behind a
    cascade reads int16 frames from the workspace."""
    in_t, hop = Q15_FORM_SUFFIX[form]
    first = None if cascade is None else _tmpl(f"{cascade[0]}_kernel", *in_t, *cascade[1], *hop)
    if call == "filter":
        assert "hop" not in form, "filter_q15 takes frames only"
        return (_tmpl("window_q15_kernel", *in_t),) if first is None else (first,)
    out, fold = Q15_CALL[call]
    if first is None:
        k = (_tmpl("fft_q15_kernel", *in_t, "true", out, *hop),)
    else:
        k = (first, _tmpl("fft_q15_kernel", "short", "false", out))
    return k + ((fold,) if fold else ())


# ------------------------------------------------------------------------------------------------- kernels without LDS
# unit -> its kernels that may be classified "exempt".  The inventory test takes the unit's resource remarks from the
# Makefile (native.remarks: the product's compiler and flags, as the resource-* targets have them) and holds each of these
# kernels to "LDS Size [bytes/block]: 0" -- and, because dynamic LDS shows as 0 in that remark (the FFT kernels prove it),
# the unit and the headers it includes to no `extern __shared__` declaration (unit_text).
NO_LDS_UNITS = {
    "cascade_q15.hip": ("window_q15_kernel<short>", "window_q15_kernel<SaP12>"),
    "trace_fold_q15.hip": ("trace_fold_q15_kernel",),
    "spectra_fold_q15.hip": ("spectra_fold_q15_kernel",),
    "sa_streams.cpp": ("sa_spin_kernel",),
}


def lds_remarks(unit):
    """{mangled function name: LDS bytes per block} of every kernel of a unit, from its resource remarks."""
    out, name = {}, None
    for ln in native.remarks(unit).splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", ln)
        if m and name is not None:
            out[name] = int(m.group(1))
    return out


def demangled_keys(mangled):
    """{mangled kernel name: its key}, demangled as inventory() has them from the symbol table."""
    names = list(mangled)
    lines = native.output_of([native.CXXFILT], input="\n".join(names), timeout=120).splitlines()
    assert len(lines) == len(names), lines
    return {m: key_of(re.sub(r"^void ", "", d)) for m, d in zip(names, lines)}


def lds_of(remarks, kernel):
    """The LDS sizes of the instantiations of `kernel` among a unit's remarks.  A plain name: every instantiation of it (an
    Itanium-mangled name holds the source name behind its length).  A key with template arguments: that instantiation
    alone, found by demangling the remarks' names to keys."""
    if "<" in kernel:
        keys = demangled_keys(remarks)
        return [v for k, v in remarks.items() if keys[k] == kernel]
    return [v for k, v in remarks.items() if f"{len(kernel)}{kernel}E" in k or f"{len(kernel)}{kernel}I" in k]


def unit_text(unit, _seen=None):
    """The text of a unit and of every header of the project it includes (by "..." includes, followed through)."""
    seen = set() if _seen is None else _seen
    path = os.path.normpath(os.path.join(CSRC, unit))
    if path in seen or not os.path.exists(path):
        return ""
    seen.add(path)
    text = open(path).read()
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M):
        text += unit_text(os.path.join(os.path.dirname(unit), inc), seen)
    return text


# ------------------------------------------------------------------------------------------------------------ the table
# iir_f64_kernel<0, InT>: process_float (specan_abi.cpp) takes the float64-state path only where `pl.k.nsec > 0`, and
# a plan's nsec is the padded section count 0, 2, 4 or 6 -- so `case 0` of launch_in (iir_f64.hip) has no caller
UNREACHABLE_F64 = "unreachable: specan_abi.cpp, process_float: `f64 = ... && cascade && pl.k.nsec > 0`"


def float_rows():
    """Every instantiation the float launchers can name -> its group: "float:bypass" without a cascade, "float:defaults" at
    the six sections of the default design (UNIT false), "float:cascades_<torch dtype>" at any other cascade."""
    rows = {}
    for dtype, in_t in CXX_IN.items():
        # launch_in (iir_f64.hip): `case 0`, `case 2`, `case 4`, `case 6` of every input type
        for nsec in (0, 2, 4, 6):
            rows[f"iir_f64_kernel<{nsec}, {in_t}>"] = "float:f64" if nsec else UNREACHABLE_F64
            # launch_chain (chain_f32.hpp): `case 0` is launch_nsec<0, false> alone, the others `unit ? <n, true> : <n, false>`
            for unit in (False, True) if nsec else (False,):
                group = "float:bypass" if nsec == 0 else "float:defaults" if nsec == 6 and not unit else f"float:cascades_{dtype}"
                # launch_nsec: SA_OUT_TIME launches time_f32_kernel<InT, NSEC, UNIT>, the four other kinds go on to
                # launch_spectrum: `ka.wingen ? <..., WG, false> : <..., false, false>` with WG = NSEC > 0, and
                # `if (one_round) kern = <InT, 0, false, ..., false, true>` under ONE_ROUND_FORM = NSEC == 0 && InT is float
                rows[_chain_kernel(dtype, nsec, unit, False, False, "time")] = group
                forms = [(False, False)] + [(True, False)] * (nsec > 0) + [(False, True)] * (nsec == 0 and in_t == "float")
                for wingen, one_round in forms:
                    for kind in ("marker", *FLOAT_OUT):
                        rows[_chain_kernel(dtype, nsec, unit, wingen, one_round, kind)] = group
    return rows


def q15_rows():
    """Every instantiation the Q15 launchers can name -> the case of test_poisoned_lds_integer_chain that launches it."""
    rows = {}
    for in_t, hop in Q15_FORM_SUFFIX.values():
        # sa_launch_fft_q15 (fft_q15.hip) names the five OUT; launch_fft_q15 below it windows packed samples and streams
        # always (<OUT, true>) and int16 frames by `apply_window ? <OUT, true> : <OUT, false>`: false behind a cascade
        for out in (0, 1, 2, 16, 128):
            rows[_tmpl("fft_q15_kernel", *in_t, "true", out, *hop)] = "q15:bypass"
            rows[_tmpl("fft_q15_kernel", "short", "false", out)] = "q15:default"
        # launch_cascade (cascade_q15.hip): `p.filter == SA_FILTER_WIDE`, else `nob1 ? <InT, true, Hop...> : <InT, false, Hop...>`
        rows[_tmpl("filter_w14_kernel", *in_t, *hop)] = "q15:wide6"
        rows[_tmpl("filter_q7_kernel", *in_t, "true", *hop)] = "q15:default"
        rows[_tmpl("filter_q7_kernel", *in_t, "false", *hop)] = "q15:custom_b1"
    return rows


TABLE = {
    **float_rows(),
    **q15_rows(),
    "sa_spin_kernel": "exempt: no LDS (sa_streams.cpp: waits on the clock, reads and writes no memory)",
    "spectra_fold_q15_kernel": "exempt: no LDS (spectra_fold_q15.hip: one bin per thread, registers only)",
    "trace_fold_q15_kernel": "exempt: no LDS (trace_fold_q15.hip: one record per thread, registers only)",
    "window_q15_kernel<short>": "exempt: no LDS (cascade_q15.hip: element-wise, eight samples per thread)",
    "window_q15_kernel<SaP12>": "exempt: no LDS (cascade_q15.hip: element-wise, eight samples per thread)",
}
