"""The one place where the tests call a compiler or a binary tool (a plain module, like gpu_support.py): the tools, each looked
up once; the compiler's resource remarks, through the Makefile that builds the product, so that they are made with its flags;
stand-alone host programs under the host sanitizers; what a header declares against what a library exports, leaves undefined
and links; and the helper objects of the GPU tests (tests/hip/*.hip).  Sanitizers are for the stand-alone programs alone:
nothing built here with them is loaded into this process."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "fpga_real_time_fft_analyzer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def _tool(*names):
    """The first of `names` on the PATH; the last one, a full path, as it stands."""
    return next((p for p in map(shutil.which, names[:-1]) if p), names[-1])


HIPCC = _tool("hipcc", "/opt/rocm/bin/hipcc")
CC = _tool("gcc", "cc", "clang", None) or shutil.which("/opt/rocm/llvm/bin/clang")        # None: no C compiler here
NM = _tool("nm", "llvm-nm", "/opt/rocm/llvm/bin/llvm-nm")
CXXFILT = _tool("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt")
LDD = _tool("ldd", "ldd")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run(cmd, timeout=300, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, **kw)


def output_of(cmd, **kw):
    """The standard output of a command that must succeed."""
    r = run(cmd, **kw)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


# ------------------------------------------------------------------------------------------------------ resource remarks
def remarks(unit):
    """The -Rpass-analysis=kernel-resource-usage stream of one unit of csrc/, from the Makefile's `remarks` target: the
    product's compiler and the product's CXXFLAGS, whatever they become."""
    return output_of(["make", "-s", "-C", CSRC, "remarks", "UNITS=" + unit], timeout=600)


# -------------------------------------------------------------------------------------------------- stand-alone programs
def standalone(tmp_path, name, units=(), sanitize=True, args=()):
    """Builds tests/cpp/<name>.cpp with the named units of csrc/ for the host alone and runs it: its standard output, the
    exit code being 0.  `sanitize`: -O1 -g with the address and undefined-behaviour sanitizers when they link here (a plain
    build otherwise: the program's own checks still run), and which of the two ran is printed; without it a plain -O2 build."""
    exe = str(tmp_path / name)
    srcs = [os.path.join(ROOT, "tests", "cpp", name + ".cpp")] + [os.path.join(CSRC, u) for u in units]
    base = [HIPCC, *(("-O1", "-g") if sanitize else ("-O2",)), "-std=c++17", "--offload-host-only", "-x", "hip", *srcs, "-o", exe]
    r = run(base + (list(SANITIZE) if sanitize else []))
    if sanitize:
        print("sanitizers:", "address,undefined" if r.returncode == 0 else "did not link here: plain build")
        if r.returncode != 0:
            r = run(base)
    assert r.returncode == 0, r.stderr
    r = run([exe, *args], timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def standalone_checks(tmp_path, name, units=(), args=()):
    """standalone() under the sanitizers for a program that ends with "ok <number of checks>": that number."""
    out = standalone(tmp_path, name, units, args=args)
    assert out.startswith("ok "), out
    return int(out.split()[1])


# -------------------------------------------------------------------------------------------------- headers and libraries
def declared(header):
    """The sa_* functions a header declares, sorted (comments dropped)."""
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(sa_[a-z0-9_]+)\s*\(", txt)))


def exported(lib):
    """The functions a shared object exports (`nm -D`, type T), sorted."""
    rows = (ln.split() for ln in output_of([NM, "-D", "--defined-only", lib]).splitlines())
    return sorted(f[2] for f in rows if len(f) == 3 and f[1] == "T")


def undefined(lib):
    """What a shared object leaves to others, as `nm -D --undefined-only` prints it."""
    return output_of([NM, "-D", "--undefined-only", lib])


def needed(lib):
    """The libraries a shared object is loaded with, as `ldd` prints them."""
    return output_of([LDD, lib])


def compiles_as_c(tmp_path, text, std="c99"):
    """`text` after the project's headers is pedantic C of that standard without a warning."""
    src = tmp_path / "use.c"
    src.write_text(text)
    output_of([CC, "-std=" + std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(src)])


def c_program_exit_code(tmp_path, text, std="c11"):
    """Compiles `text` against the project's headers as a C program and runs it: its exit code."""
    src, exe = tmp_path / "m.c", str(tmp_path / "m")
    src.write_text(text)
    output_of([CC, "-std=" + std, "-I", INCLUDE, str(src), "-o", exe])
    return subprocess.call([exe])


def link_c_caller(source, exe, pkg):
    """A C program of tests/c/ linked against libspecan_hip.so in `pkg` and the HIP runtime, as a user of the library would."""
    assert CC, "a C compiler is part of the image"
    output_of([CC, "-O2", "-Wall", "-Werror", "-std=c11", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + INCLUDE, source,
               "-L" + pkg, "-lspecan_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib",
               "-o", exe])
    return exe


# ----------------------------------------------------------------------------------------------------- GPU helper objects
def gpu_helper(directory, name):
    """tests/hip/<name>.hip as a shared object for gfx950 in `directory` (not part of the library): its path."""
    so = str(directory / f"lib{name}.so")
    output_of([HIPCC, "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hip", name + ".hip"), "-o", so])
    return so


class Lds:
    """lds_fill / lds_probe of tests/hip/lds_fill.hip on the current torch stream, over a grid of 8 workgroups per CU."""

    def __init__(self, so, torch):
        self.torch = torch
        L = ctypes.CDLL(so)                    # torch is imported: the helper binds to the HIP runtime torch mapped
        L.lds_fill.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        L.lds_probe.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.lds_fill.restype = L.lds_probe.restype = ctypes.c_int
        self.L = L
        self.grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count
        self.counts = torch.empty(self.grid * 4, dtype=torch.int32, device="cuda")

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def fill(self, word):
        rc = self.L.lds_fill(word, self.grid, self._stream())
        assert rc == 0, f"lds_fill: hipError {rc}"

    def probe(self, word):
        """Words differing from `word`, one count per probe wave (-1 stays where a wave stored nothing)."""
        self.counts.fill_(-1)
        rc = self.L.lds_probe(word, self.grid, self.counts.data_ptr(), self._stream())
        assert rc == 0, f"lds_probe: hipError {rc}"
        return self.counts.cpu().numpy().view(np.uint32)
