"""Shared by tests/test_gpu_isolation.py (a plain module, like structured_cases.py): the kernel instantiations of the built
library, read from its symbol table, the names the isolation tests' variant tuples stand for, and the committed table that
says of every instantiation how the suite knows it does not read LDS words it did not write.

hipcc emits one host function `__device_stub__<kernel>` per kernel instantiation of a unit; `nm -C` lists them demangled.
The key used here is the kernel's name with its template arguments and without its argument list, the anonymous namespace
dropped: "fft_q15_kernel<short, false, 128>", "chain_f32_kernel<SaP12, 4, true, 0, false, false, float>",
"filter_w14_kernel<short, int>".

TABLE classifies every key as exactly one of
  "float:<group>"       poisoned by test_poisoned_lds_float_chain[<group>]: the group's variant set holds a tuple whose
                        launches (float_kernels) include the key;
  "q15:<case>"          poisoned by test_poisoned_lds_integer_chain[<case>], likewise (q15_kernels);
  "exempt: <why>"       uses no LDS at all -- proven by the inventory test from the compiler's resource remarks and the
                        unit's source (NO_LDS_UNITS), never taken on trust;
  "unreachable: <why>"  built, but no public call launches it: <why> names the dispatch line.
A kernel added to the library (or removed from it) fails tests/test_gpu_isolation.py::test_kernel_inventory_is_classified
without a GPU until it has a row here -- and a "float:" / "q15:" row holds only if that case's pinned variant set, which
the GPU test asserts equal to what it launched, contains the kernel."""
import os
import re
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "fpga_real_time_fft_analyzer_amd", "csrc")
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
    """The keys of every kernel instantiation in the shared object, from `nm -C` (local symbols included)."""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-C", lib_path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    keys = [normalise(ln.split(None, 2)[2]) for ln in r.stdout.splitlines() if STUB in ln and len(ln.split(None, 2)) == 3]
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
# unit -> its kernels that may be classified "exempt".  The inventory test compiles the unit for gfx950 to /dev/null with
# the resource remarks on, as the Makefile's resource-* targets do, and holds each of these kernels to
# "LDS Size [bytes/block]: 0" -- and, because dynamic LDS shows as 0 in that remark (the FFT kernels prove it), the unit
# and the headers it includes to no `extern __shared__` declaration (unit_text).
NO_LDS_UNITS = {
    "cascade_q15.hip": ("window_q15_kernel<short>", "window_q15_kernel<SaP12>"),
    "trace_fold_q15.hip": ("trace_fold_q15_kernel",),
    "spectra_fold_q15.hip": ("spectra_fold_q15_kernel",),
    "sa_streams.cpp": ("sa_spin_kernel",),
}
HIPCC_FLAGS = ("-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-x", "hip", "-c")


def lds_remarks(unit):
    """{mangled function name: LDS bytes per block} of every kernel of a unit, from -Rpass-analysis=kernel-resource-usage."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, *HIPCC_FLAGS, unit, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", ln)
        if m and name is not None:
            out[name] = int(m.group(1))
    return out


def demangled_keys(mangled):
    """{mangled kernel name: its key} through c++filt, as inventory() has them from `nm -C`."""
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    names = list(mangled)
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == len(names), r.stderr
    return {m: key_of(re.sub(r"^void ", "", d)) for m, d in zip(names, r.stdout.splitlines())}


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
TABLE = {
    "chain_f32_kernel<SaP12, 0, false, 0, false, false, float>": "float:bypass",
    "chain_f32_kernel<SaP12, 0, false, 1, false, false, float>": "float:bypass",
    "chain_f32_kernel<SaP12, 0, false, 2, false, false, float>": "float:bypass",
    "chain_f32_kernel<SaP12, 2, false, 0, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, false, 0, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, false, 1, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, false, 1, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, false, 2, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, false, 2, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, true, 0, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, true, 0, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, true, 1, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, true, 1, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, true, 2, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 2, true, 2, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, false, 0, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, false, 0, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, false, 1, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, false, 1, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, false, 2, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, false, 2, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, true, 0, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, true, 0, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, true, 1, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, true, 1, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, true, 2, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 4, true, 2, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 6, false, 0, false, false, float>": "float:defaults",
    "chain_f32_kernel<SaP12, 6, false, 0, true, false, float>": "float:defaults",
    "chain_f32_kernel<SaP12, 6, false, 1, false, false, float>": "float:defaults",
    "chain_f32_kernel<SaP12, 6, false, 1, true, false, float>": "float:defaults",
    "chain_f32_kernel<SaP12, 6, false, 2, false, false, float>": "float:defaults",
    "chain_f32_kernel<SaP12, 6, false, 2, true, false, float>": "float:defaults",
    "chain_f32_kernel<SaP12, 6, true, 0, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 6, true, 0, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 6, true, 1, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 6, true, 1, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 6, true, 2, false, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<SaP12, 6, true, 2, true, false, float>": "float:cascades_uint8",
    "chain_f32_kernel<float, 0, false, 0, false, false>": "float:bypass",
    "chain_f32_kernel<float, 0, false, 0, false, true>": "float:bypass",
    "chain_f32_kernel<float, 0, false, 1, false, false>": "float:bypass",
    "chain_f32_kernel<float, 0, false, 1, false, true>": "float:bypass",
    "chain_f32_kernel<float, 0, false, 2, false, false>": "float:bypass",
    "chain_f32_kernel<float, 0, false, 2, false, true>": "float:bypass",
    "chain_f32_kernel<float, 2, false, 0, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, false, 0, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, false, 1, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, false, 1, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, false, 2, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, false, 2, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, true, 0, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, true, 0, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, true, 1, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, true, 1, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, true, 2, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 2, true, 2, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, false, 0, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, false, 0, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, false, 1, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, false, 1, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, false, 2, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, false, 2, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, true, 0, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, true, 0, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, true, 1, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, true, 1, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, true, 2, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 4, true, 2, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 6, false, 0, false, false>": "float:defaults",
    "chain_f32_kernel<float, 6, false, 0, true, false>": "float:defaults",
    "chain_f32_kernel<float, 6, false, 1, false, false>": "float:defaults",
    "chain_f32_kernel<float, 6, false, 1, true, false>": "float:defaults",
    "chain_f32_kernel<float, 6, false, 2, false, false>": "float:defaults",
    "chain_f32_kernel<float, 6, false, 2, true, false>": "float:defaults",
    "chain_f32_kernel<float, 6, true, 0, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 6, true, 0, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 6, true, 1, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 6, true, 1, true, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 6, true, 2, false, false>": "float:cascades_float32",
    "chain_f32_kernel<float, 6, true, 2, true, false>": "float:cascades_float32",
    "chain_f32_kernel<short, 0, false, 0, false, false, float>": "float:bypass",
    "chain_f32_kernel<short, 0, false, 1, false, false, float>": "float:bypass",
    "chain_f32_kernel<short, 0, false, 2, false, false, float>": "float:bypass",
    "chain_f32_kernel<short, 2, false, 0, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, false, 0, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, false, 1, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, false, 1, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, false, 2, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, false, 2, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, true, 0, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, true, 0, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, true, 1, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, true, 1, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, true, 2, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 2, true, 2, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, false, 0, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, false, 0, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, false, 1, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, false, 1, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, false, 2, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, false, 2, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, true, 0, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, true, 0, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, true, 1, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, true, 1, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, true, 2, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 4, true, 2, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 6, false, 0, false, false, float>": "float:defaults",
    "chain_f32_kernel<short, 6, false, 0, true, false, float>": "float:defaults",
    "chain_f32_kernel<short, 6, false, 1, false, false, float>": "float:defaults",
    "chain_f32_kernel<short, 6, false, 1, true, false, float>": "float:defaults",
    "chain_f32_kernel<short, 6, false, 2, false, false, float>": "float:defaults",
    "chain_f32_kernel<short, 6, false, 2, true, false, float>": "float:defaults",
    "chain_f32_kernel<short, 6, true, 0, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 6, true, 0, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 6, true, 1, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 6, true, 1, true, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 6, true, 2, false, false, float>": "float:cascades_int16",
    "chain_f32_kernel<short, 6, true, 2, true, false, float>": "float:cascades_int16",
    "chain_marker_kernel<SaP12, 0, false, false, false, float>": "float:bypass",
    "chain_marker_kernel<SaP12, 2, false, false, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 2, false, true, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 2, true, false, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 2, true, true, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 4, false, false, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 4, false, true, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 4, true, false, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 4, true, true, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 6, false, false, false, float>": "float:defaults",
    "chain_marker_kernel<SaP12, 6, false, true, false, float>": "float:defaults",
    "chain_marker_kernel<SaP12, 6, true, false, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<SaP12, 6, true, true, false, float>": "float:cascades_uint8",
    "chain_marker_kernel<float, 0, false, false, false>": "float:bypass",
    "chain_marker_kernel<float, 0, false, false, true>": "float:bypass",
    "chain_marker_kernel<float, 2, false, false, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 2, false, true, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 2, true, false, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 2, true, true, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 4, false, false, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 4, false, true, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 4, true, false, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 4, true, true, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 6, false, false, false>": "float:defaults",
    "chain_marker_kernel<float, 6, false, true, false>": "float:defaults",
    "chain_marker_kernel<float, 6, true, false, false>": "float:cascades_float32",
    "chain_marker_kernel<float, 6, true, true, false>": "float:cascades_float32",
    "chain_marker_kernel<short, 0, false, false, false, float>": "float:bypass",
    "chain_marker_kernel<short, 2, false, false, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 2, false, true, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 2, true, false, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 2, true, true, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 4, false, false, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 4, false, true, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 4, true, false, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 4, true, true, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 6, false, false, false, float>": "float:defaults",
    "chain_marker_kernel<short, 6, false, true, false, float>": "float:defaults",
    "chain_marker_kernel<short, 6, true, false, false, float>": "float:cascades_int16",
    "chain_marker_kernel<short, 6, true, true, false, float>": "float:cascades_int16",
    "fft_q15_kernel<short, true, 0, int>": "q15:bypass",
    "fft_q15_kernel<short, true, 128, int>": "q15:bypass",
    "fft_q15_kernel<short, true, 16, int>": "q15:bypass",
    "fft_q15_kernel<short, true, 1, int>": "q15:bypass",
    "fft_q15_kernel<short, true, 2, int>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 0, int>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 128, int>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 16, int>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 1, int>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 2, int>": "q15:bypass",
    "fft_q15_kernel<short, false, 0>": "q15:default",
    "fft_q15_kernel<short, false, 128>": "q15:default",
    "fft_q15_kernel<short, false, 16>": "q15:default",
    "fft_q15_kernel<short, false, 1>": "q15:default",
    "fft_q15_kernel<short, false, 2>": "q15:default",
    "fft_q15_kernel<short, true, 0>": "q15:bypass",
    "fft_q15_kernel<short, true, 128>": "q15:bypass",
    "fft_q15_kernel<short, true, 16>": "q15:bypass",
    "fft_q15_kernel<short, true, 1>": "q15:bypass",
    "fft_q15_kernel<short, true, 2>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 0>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 128>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 16>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 1>": "q15:bypass",
    "fft_q15_kernel<SaP12, true, 2>": "q15:bypass",
    "filter_q7_kernel<short, false, int>": "q15:custom_b1",
    "filter_q7_kernel<short, true, int>": "q15:default",
    "filter_q7_kernel<SaP12, false, int>": "q15:custom_b1",
    "filter_q7_kernel<SaP12, true, int>": "q15:default",
    "filter_q7_kernel<short, false>": "q15:custom_b1",
    "filter_q7_kernel<short, true>": "q15:default",
    "filter_q7_kernel<SaP12, false>": "q15:custom_b1",
    "filter_q7_kernel<SaP12, true>": "q15:default",
    "filter_w14_kernel<short, int>": "q15:wide6",
    "filter_w14_kernel<SaP12, int>": "q15:wide6",
    "filter_w14_kernel<short>": "q15:wide6",
    "filter_w14_kernel<SaP12>": "q15:wide6",
    "iir_f64_kernel<0, SaP12>": UNREACHABLE_F64,
    "iir_f64_kernel<0, float>": UNREACHABLE_F64,
    "iir_f64_kernel<0, short>": UNREACHABLE_F64,
    "iir_f64_kernel<2, SaP12>": "float:f64",
    "iir_f64_kernel<2, float>": "float:f64",
    "iir_f64_kernel<2, short>": "float:f64",
    "iir_f64_kernel<4, SaP12>": "float:f64",
    "iir_f64_kernel<4, float>": "float:f64",
    "iir_f64_kernel<4, short>": "float:f64",
    "iir_f64_kernel<6, SaP12>": "float:f64",
    "iir_f64_kernel<6, float>": "float:f64",
    "iir_f64_kernel<6, short>": "float:f64",
    "sa_spin_kernel": "exempt: no LDS (sa_streams.cpp: waits on the clock, reads and writes no memory)",
    "spectra_fold_q15_kernel": "exempt: no LDS (spectra_fold_q15.hip: one bin per thread, registers only)",
    "time_f32_kernel<SaP12, 0, false, float>": "float:bypass",
    "time_f32_kernel<SaP12, 2, false, float>": "float:cascades_uint8",
    "time_f32_kernel<SaP12, 2, true, float>": "float:cascades_uint8",
    "time_f32_kernel<SaP12, 4, false, float>": "float:cascades_uint8",
    "time_f32_kernel<SaP12, 4, true, float>": "float:cascades_uint8",
    "time_f32_kernel<SaP12, 6, false, float>": "float:defaults",
    "time_f32_kernel<SaP12, 6, true, float>": "float:cascades_uint8",
    "time_f32_kernel<float, 0, false>": "float:bypass",
    "time_f32_kernel<float, 2, false>": "float:cascades_float32",
    "time_f32_kernel<float, 2, true>": "float:cascades_float32",
    "time_f32_kernel<float, 4, false>": "float:cascades_float32",
    "time_f32_kernel<float, 4, true>": "float:cascades_float32",
    "time_f32_kernel<float, 6, false>": "float:defaults",
    "time_f32_kernel<float, 6, true>": "float:cascades_float32",
    "time_f32_kernel<short, 0, false, float>": "float:bypass",
    "time_f32_kernel<short, 2, false, float>": "float:cascades_int16",
    "time_f32_kernel<short, 2, true, float>": "float:cascades_int16",
    "time_f32_kernel<short, 4, false, float>": "float:cascades_int16",
    "time_f32_kernel<short, 4, true, float>": "float:cascades_int16",
    "time_f32_kernel<short, 6, false, float>": "float:defaults",
    "time_f32_kernel<short, 6, true, float>": "float:cascades_int16",
    "trace_fold_q15_kernel": "exempt: no LDS (trace_fold_q15.hip: one record per thread, registers only)",
    "window_q15_kernel<short>": "exempt: no LDS (cascade_q15.hip: element-wise, eight samples per thread)",
    "window_q15_kernel<SaP12>": "exempt: no LDS (cascade_q15.hip: element-wise, eight samples per thread)",
}
