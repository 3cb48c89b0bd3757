"""Shared by the tests of the handle-less reduction libraries (a plain module, like q15_cases.py, native.py and
kernel_inventory.py): LIBRARIES, one row of data per libspecan_x.so in the order of abi.LIBRARIES, which
tests/test_reduction_libraries_cpu.py holds every library to; the names derived from a row's short name; and the constants
and helpers that tests/test_f32_x_cpu.py and tests/test_gpu_f32_x.py of several libraries use alike.

A row says what is x's own.  Everything else follows from the short name: include/specan_x.h, libspecan_x.so beside
libspecan_hip.so, abi.X_SIGNATURES, abi.X_LIB_PATH, abi.x_lib, and the Makefile's X_SRCS, X_OUT, X_OBJS and resource-x-f32.

  names      the four exported functions, sorted
  units      the two units of csrc/, the kernel unit first
  remarks    kernel name -> (resource remarks it must show, least and most static LDS in bytes per block of each)
  occupancy, vgprs_max   where the library promises them: the waves per SIMD of every kernel, the most VGPRs of any
  launches   hipLaunchKernelGGL in the kernel unit
  fp_contract_off        `#pragma clang fp contract(off)` must stand in the kernel unit
  absent     words that must not stand in the kernel unit, and `counts`: word -> how often it must stand there; both are
             read on the unit without its // comments.  `comment` is text the words may stand in: peaks' "No atomics"
             stands in a // comment and is gone before the words are looked for, so the entry is kept as a record only
  design     the section of DESIGN.md that records the figures of the remarks
"""
import os

import numpy as np

from conftest import N
from native import INCLUDE

SA_OK, SA_EINVAL, SA_ESHAPE = 0, -1, -2
BASE = (1 << 47) - (1 << 36)
FIELDS = (None, "peak", "power")

QUIET = ("atomic", "s_setreg", "denorm", "hipMemset")

LIBRARIES = {
    "fold": dict(
        names=["sa_fold_check", "sa_fold_last_error", "sa_fold_mag_f32", "sa_fold_version"],
        units=("fold_mag_f32.hip", "sa_fold_check.cpp"),
        remarks={"fold_mag_f32_kernel": (7, 0, 0)},                # no LDS: the bins are folded in registers and DPP moves
        launches=1, fp_contract_off=False, absent=QUIET, design="4.16"),
    "peaks": dict(
        names=["sa_peaks_check", "sa_peaks_f32", "sa_peaks_last_error", "sa_peaks_version"],
        units=("peaks_f32.hip", "sa_peaks_check.cpp"),
        remarks={"peaks_f32_kernel": (3, 80, 80)},                 # the four wave slots (two buffers) and the four counts
        launches=1, fp_contract_off=False, absent=QUIET, comment=("No atomics",), design="4.17"),
    "rank": dict(
        names=["sa_rank_check", "sa_rank_f32", "sa_rank_last_error", "sa_rank_version"],
        units=("rank_f32.hip", "sa_rank_check.cpp"),
        remarks={"rank_f32_kernel": (3, 256, 256)},                # the count words: two buffers of eight ranks by four waves
        launches=1, fp_contract_off=False, absent=QUIET, design="4.18"),
    "hist": dict(
        names=["sa_hist_check", "sa_hist_f32", "sa_hist_last_error", "sa_hist_version"],
        units=("hist_f32.hip", "sa_hist_check.cpp"),
        # the count: 64 levels of 257 counters and the 64 words of the edge tree, at 64 VGPRs or fewer and occupancy 8 --
        # two workgroups of 16 waves on a compute unit; the kernel that zeroes the output of the sliced form uses none
        remarks={"hist_f32_kernel": (6, 66048, 66048), "hist_zero_kernel": (1, 0, 0)}, occupancy=8, vgprs_max=64,
        launches=2, fp_contract_off=False, absent=("atomicAdd(", "s_setreg", "denorm", "hipMalloc", "hipMemset"),
        counts={"__hip_atomic_fetch_add(": 2},                     # one LDS add, one merge: unsigned
        design="4.19"),
    "bands": dict(
        names=["sa_bands_check", "sa_bands_f32", "sa_bands_last_error", "sa_bands_version"],
        units=("bands_f32.hip", "sa_bands_check.cpp"),
        remarks={"bands_f32_kernel": (6, 1, 8192)}, launches=2, fp_contract_off=True, absent=QUIET, design="4.20"),
    "mask": dict(
        names=["sa_mask_check", "sa_mask_f32", "sa_mask_last_error", "sa_mask_version"],
        units=("mask_f32.hip", "sa_mask_check.cpp"),
        remarks={"mask_f32_kernel": (9, 1, 1024), "mask_summary_kernel": (1, 1, 1024)},
        launches=2,                                                # the row launch, written once for the nine, and the summary
        fp_contract_off=False, absent=QUIET, design="4.21"),
    "harm": dict(
        names=["sa_harm_check", "sa_harm_f32", "sa_harm_last_error", "sa_harm_version"],
        units=("harm_f32.hip", "sa_harm_check.cpp"),
        remarks={"harm_f32_kernel": (3, 1, 2048)}, launches=1, fp_contract_off=True, absent=QUIET, design="4.22"),
    "cfar": dict(
        names=["sa_cfar_check", "sa_cfar_f32", "sa_cfar_last_error", "sa_cfar_version"],
        units=("cfar_f32.hip", "sa_cfar_check.cpp"),
        remarks={"cfar_f32_kernel": (3, 1, 160 * 1024 // 2)},      # small enough for more than one workgroup on a CU (160 KiB)
        launches=1, fp_contract_off=True, absent=QUIET, design="4.24"),
    "signals": dict(
        names=["sa_signals_check", "sa_signals_f32", "sa_signals_last_error", "sa_signals_version"],
        units=("signals_f32.hip", "sa_signals_check.cpp"),
        remarks={"signals_f32_kernel": (3, 1, 8192)}, launches=1, fp_contract_off=True, absent=QUIET, design="4.23"),
}


# ------------------------------------------------------------------------------------------- what follows from the name
def header(x):
    return os.path.join(INCLUDE, f"specan_{x}.h")


def signatures(x):
    from fpga_real_time_fft_analyzer_amd import abi
    return getattr(abi, f"{x.upper()}_SIGNATURES")


def lib_path(x):
    from fpga_real_time_fft_analyzer_amd import abi
    return getattr(abi, f"{x.upper()}_LIB_PATH")


def built(x):
    """libspecan_x.so, built on demand by the package's one build step (it cross-compiles without a GPU)."""
    from fpga_real_time_fft_analyzer_amd import abi
    if not os.path.exists(lib_path(x)):
        abi.build()
    return getattr(abi, f"{x}_lib")()


# ------------------------------------------------------------------------------------- shared by the libraries' own tests
def _shared(a):
    a.setflags(write=False)                                       # computed once, shared by the tests of both files
    return a


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def key(v):
    """the key of one value: its float32 bits with the sign cleared"""
    return int(bits(np.float32(v)).ravel()[0]) & 0x7FFFFFFF


def records_of(pts, field):
    """``pts`` float32 [R, N] in the layout of ``field``: itself, or records whose other float is a NaN"""
    if field is None:
        return pts
    rec = np.full(pts.shape + (2,), np.nan, np.float32)
    rec[..., 0 if field == "peak" else 1] = pts
    return rec


def planted(pairs, fill=0.0, rows=1):
    """rows equal rows of `fill` with the (bin, value) pairs planted"""
    r = np.full((rows, N), fill, np.float32)
    for b, v in pairs:
        r[:, b] = v
    return r
