"""ctypes binding of ``libspecan_hip.so`` (the C ABI declared in ``include/specan.h`` and ``include/specan_ext.h``) and of the
handle-less libraries of the table ``LIBRARIES``: for every short name ``x`` there, ``libspecan_x.so`` declared in
``include/specan_x.h``, its path ``X_LIB_PATH``, its entry points ``X_SIGNATURES`` and its loader ``x_lib()``.

This is the only place the shared libraries are loaded.  There is no CPU fallback: if the
library is missing the import of any compute entry point raises, and creating a handle
itself fails when no HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libspecan_hip.so")
CSRC = os.path.join(_PKG, "csrc")

# error codes / constants (include/specan.h)
SA_OK, SA_EINVAL, SA_ESHAPE, SA_EHIP, SA_ESTATE, SA_ENOMEM = 0, -1, -2, -3, -4, -5
SA_N = 16384
SA_FRAME_BYTES = 65536
SA_P12_FRAME_BYTES = 24576       # packed 12-bit samples: 3 bytes per 2 samples
SA_FILTER_DEFAULT, SA_FILTER_CUSTOM, SA_FILTER_NONE, SA_FILTER_WIDE = 0x00, 0xA1, 0xB1, 0xA2
SA_WIN_RTL_SIGNED, SA_WIN_HANN_U16 = 0, 1
SA_OUT_MAG_FULL, SA_OUT_MAG_HALF, SA_OUT_SPEC_HALF, SA_OUT_TIME, SA_OUT_MARKER = 0, 1, 2, 3, 4
SA_Q15_OUT_IQ, SA_Q15_OUT_MAG, SA_Q15_OUT_MARKER = 0, 1, 2
SA_Q15_TRACE_LOG2W_MIN, SA_Q15_TRACE_LOG2W_MAX = 1, 6
SA_PRECISION_F32, SA_PRECISION_F64_STATE = 0, 1
# the entry points as sa_debug_check_pointers numbers them (SA_ENTRY_* of include/specan.h)
SA_ENTRIES = ("sa_process_f32", "sa_process_f32_i16", "sa_process_f32_p12", "sa_process_q15", "sa_process_q15_out",
              "sa_process_q15_p12", "sa_filter_q15", "sa_filter_q15_p12")


def SA_Q15_TRACE_KIND(log2w: int) -> int:
    """The out_kind of the Q15 chain's display trace with buckets of 2**log2w bins (the macro of include/specan.h)."""
    return 0x10 | log2w


SA_Q15_TRACE_LOG2A_MIN, SA_Q15_TRACE_LOG2A_MAX = 1, 7


def SA_Q15_TRACE_AVG_KIND(log2w: int, log2a: int) -> int:
    """The out_kind of the Q15 chain's trace over buckets of 2**log2w bins and groups of 2**log2a consecutive frames (the macro
    of include/specan.h): max hold and summed power, one record per bucket and group."""
    return 0x80 | log2a << 3 | log2w


SA_Q15_HOP_FIELD_MAX = 2048


def SA_Q15_HOP_KIND(kind: int, hop: int) -> int:
    """The out_kind word of sa_process_q15_out / sa_process_q15_p12 for frames cut from one sample stream ``hop`` samples
    apart (the macro of include/specan.h): the kind in bits 0..7, hop / 8 in bits 8..19.  hop = 0 is the kind itself."""
    return kind | (hop // 8) << 8


class CmdEvents(C.Structure):
    """sa_cmd_events of include/specan.h."""
    _fields_ = [("n_start", C.c_int), ("n_uart_request", C.c_int), ("n_reset", C.c_int), ("n_uploads", C.c_int),
                ("control_changed", C.c_int), ("transport", C.c_uint8)]


class MarkerQ15(C.Structure):
    """sa_marker_q15 of include/specan.h: one SA_Q15_OUT_MARKER record, 16 bytes."""
    _fields_ = [("peak_mag", C.c_float), ("peak_bin", C.c_int32), ("band_power", C.c_uint64)]


class TracePointQ15(C.Structure):
    """sa_trace_point_q15 of include/specan.h: one record of SA_Q15_TRACE_KIND(k), 8 bytes."""
    _fields_ = [("peak_mag", C.c_float), ("power", C.c_float)]


class SpecanError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"specan error {code}: {msg}")
        self.code = code


def build(verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU): LIB_PATH and the library of every
    row of LIBRARIES are the Makefile's first target."""
    cmd = ["make", "-j4", "-C", CSRC]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


H = C.c_void_p
_P = C.POINTER
_INT = C.c_int
# the one list of entry points: name -> (restype, argtypes), name for name the declarations of include/specan.h
# (tests/test_abi_symbols.py holds the key set against the header)
SIGNATURES = {
    "sa_create": (_INT, [_INT, _P(H)]),
    "sa_destroy": (_INT, [H]),
    "sa_abi_version": (_INT, []),
    "sa_last_error": (C.c_char_p, [H]),
    "sa_reserve": (_INT, [H, _INT]),
    "sa_set_overlap": (_INT, [H, _INT]),
    "sa_get_overlap": (_INT, [H, _P(_INT)]),
    "sa_debug_overlap_streams": (_INT, [H, C.c_void_p, _P(_INT)]),
    "sa_flush": (_INT, [H, C.c_void_p]),
    "sa_set_profiling": (_INT, [H, _INT]),
    "sa_profile_read": (_INT, [H, _P(C.c_float), _INT]),
    "sa_set_filter_mode": (_INT, [H, C.c_uint8]),
    "sa_get_filter_mode": (_INT, [H, _P(C.c_uint8)]),
    "sa_load_coeffs_q7": (_INT, [H, _P(C.c_int8)]),
    "sa_get_coeffs_q7": (_INT, [H, _P(C.c_int8)]),
    "sa_feed_command_bytes": (_INT, [H, _P(C.c_uint8), C.c_size_t, _P(_INT)]),
    "sa_feed_command_bytes_ex": (_INT, [H, _P(C.c_uint8), C.c_size_t, _P(CmdEvents)]),
    "sa_get_transport": (_INT, [H, _P(C.c_uint8)]),
    "sa_load_sos_f32": (_INT, [H, _P(C.c_float), _INT]),
    "sa_load_sos_f64": (_INT, [H, _P(C.c_double), _INT]),
    "sa_load_sos_q14": (_INT, [H, _P(C.c_int16), _INT]),
    "sa_set_window_q15": (_INT, [H, _P(C.c_int16)]),
    "sa_set_window_f32": (_INT, [H, _P(C.c_float)]),
    "sa_set_window_mode_q15": (_INT, [H, _INT]),
    "sa_get_window_q15": (_INT, [H, _P(C.c_int16)]),
    "sa_process_q15": (_INT, [H, C.c_void_p, C.c_void_p, _INT, C.c_void_p]),
    "sa_process_q15_out": (_INT, [H, C.c_void_p, C.c_void_p, _INT, _INT, C.c_void_p]),
    "sa_filter_q15": (_INT, [H, C.c_void_p, C.c_void_p, _INT, C.c_void_p]),
    "sa_process_q15_p12": (_INT, [H, C.c_void_p, C.c_void_p, _INT, _INT, C.c_void_p]),
    "sa_filter_q15_p12": (_INT, [H, C.c_void_p, C.c_void_p, _INT, C.c_void_p]),
    "sa_process_f32": (_INT, [H, C.c_void_p, C.c_void_p, _INT, _INT, C.c_void_p]),
    "sa_process_f32_i16": (_INT, [H, C.c_void_p, C.c_float, C.c_void_p, _INT, _INT, C.c_void_p]),
    "sa_process_f32_p12": (_INT, [H, C.c_void_p, C.c_float, C.c_void_p, _INT, _INT, C.c_void_p]),
    "sa_pack_samples_p12": (_INT, [_P(C.c_int16), C.c_size_t, _P(C.c_uint8)]),
    "sa_unpack_samples_p12": (_INT, [_P(C.c_uint8), C.c_size_t, _P(C.c_int16)]),
    "sa_debug_check_pointers": (_INT, [_INT, _INT, C.c_uint64, C.c_uint64, _INT]),
    "sa_pack_frame": (_INT, [_P(C.c_int16), _P(C.c_uint8)]),
    "sa_debug_iir_plan_f32": (_INT, [H, _P(C.c_float), _INT]),
    "sa_iir_plan_from_sos": (_INT, [_P(C.c_double), _INT, _P(C.c_float), _INT]),
    "sa_set_precision": (_INT, [H, _INT]),
    "sa_get_precision": (_INT, [H, _P(_INT)]),
    "sa_debug_iir_plan_f64": (_INT, [H, _P(C.c_double), _INT]),
    "sa_iir_plan_from_sos_f64": (_INT, [_P(C.c_double), _INT, _P(C.c_double), _INT]),
    "sa_set_marker_range": (_INT, [H, _INT, _INT]),
    "sa_get_marker_range": (_INT, [H, _P(_INT), _P(_INT)]),
}

# the entry points of include/specan_ext.h, data-plane calls added after the version-4 surface of include/specan.h closed:
# a table of their own, bound by lib() like the one above and held name for name against that header
# (tests/test_q15_spectra_cpu.py); no name is in both
SA_EXT_VERSION = 1
SA_EXT_ENTRIES = ("sa_spectra_q15", "sa_spectra_q15_p12", "sa_fold_iq_q15")     # as sa_ext_check_pointers numbers them
EXT_SIGNATURES = {
    "sa_ext_version": (_INT, []),
    "sa_spectra_q15": (_INT, [H, C.c_void_p, C.c_void_p, _INT, _INT, _INT, C.c_void_p]),
    "sa_spectra_q15_p12": (_INT, [H, C.c_void_p, C.c_void_p, _INT, _INT, _INT, C.c_void_p]),
    "sa_fold_iq_q15": (_INT, [H, C.c_void_p, C.c_void_p, _INT, _INT, C.c_void_p]),
    "sa_ext_check_pointers": (_INT, [_INT, _INT, _INT, C.c_uint64, C.c_uint64, _INT]),
}

# the entry points of include/specan_fold.h: libspecan_fold.so, a second product library without a handle (the fold of float
# magnitudes over groups of frames and buckets of bins), bound by fold_lib() and held name for name against that header
# (tests/test_f32_fold_cpu.py); no name is in the two tables above
SA_FOLD_VERSION = 1
SA_FOLD_LOG2A_MAX, SA_FOLD_LOG2W_MAX = 7, 6
FOLD_SIGNATURES = {
    "sa_fold_version": (_INT, []),
    "sa_fold_mag_f32": (_INT, [C.c_void_p, C.c_void_p, _INT, _INT, _INT, C.c_void_p]),
    "sa_fold_check": (_INT, [_INT, _INT, C.c_uint64, C.c_uint64, _INT]),
    "sa_fold_last_error": (C.c_char_p, []),
}

# the entry points of include/specan_peaks.h: libspecan_peaks.so, the third product library, again without a handle (the K
# strongest local maxima of each row of 16384 points), bound by peaks_lib() and held name for name against that header
# (tests/test_f32_peaks_cpu.py); no name is in the three tables above
SA_PEAKS_VERSION = 1
SA_PEAKS_K_MAX = 32
SA_PEAKS_IN_MAG, SA_PEAKS_IN_POINT_PEAK, SA_PEAKS_IN_POINT_POWER = 0, 1, 2
PEAKS_SIGNATURES = {
    "sa_peaks_version": (_INT, []),
    "sa_peaks_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, C.c_void_p, _INT, _INT, C.c_float, _INT, _INT, _INT, C.c_void_p]),
    "sa_peaks_check": (_INT, [_INT, C.c_uint64, C.c_uint64, C.c_uint64, _INT, _INT, C.c_uint32, _INT, _INT, _INT]),
    "sa_peaks_last_error": (C.c_char_p, []),
}

# the entry points of include/specan_rank.h: libspecan_rank.so, the fourth product library, again without a handle (the keys
# at given ranks of the sorted bins of each row of 16384 points), bound by rank_lib() and held name for name against that
# header (tests/test_f32_rank_cpu.py); no name is in the four tables above
SA_RANK_VERSION = 1
SA_RANK_Q_MAX = 8
SA_RANK_IN_MAG, SA_RANK_IN_POINT_PEAK, SA_RANK_IN_POINT_POWER = 0, 1, 2
RANK_SIGNATURES = {
    "sa_rank_version": (_INT, []),
    "sa_rank_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, _INT, _INT, _P(C.c_int32), _INT, _INT, C.c_void_p]),
    "sa_rank_check": (_INT, [_INT, C.c_uint64, C.c_uint64, _INT, _INT, _P(C.c_int32), _INT, _INT]),
    "sa_rank_last_error": (C.c_char_p, []),
}

# the entry points of include/specan_hist.h: libspecan_hist.so, the fifth product library, again without a handle (the count
# per group of rows, column of bins and amplitude level), bound by hist_lib() and held name for name against that header
# (tests/test_f32_hist_cpu.py); no name is in the five tables above
SA_HIST_VERSION = 1
SA_HIST_LEVELS_MAX = 64
HIST_SIGNATURES = {
    "sa_hist_version": (_INT, []),
    "sa_hist_f32": (_INT, [C.c_void_p, C.c_void_p, _INT, _INT, _INT, _INT, _P(C.c_float), _INT, _INT, C.c_void_p]),
    "sa_hist_check": (_INT, [C.c_uint64, C.c_uint64, _INT, _INT, _INT, _INT, _P(C.c_float), _INT, _INT]),
    "sa_hist_last_error": (C.c_char_p, []),
}


class Band(C.Structure):
    """sa_band of include/specan_bands.h: the bins [lo, hi) of one band, 8 bytes."""
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32)]


# the entry points of include/specan_bands.h: libspecan_bands.so, the sixth product library, again without a handle (the
# float64 power of bands of bins of each row of 16384 points and the bins at which its cumulative power crosses given
# fractions), bound by bands_lib() and held name for name against that header (tests/test_f32_bands_cpu.py); no name is in the
# tables above
SA_BANDS_VERSION = 1
SA_BANDS_MAX, SA_BANDS_Q_MAX = 16, 4
SA_BANDS_IN_MAG, SA_BANDS_IN_POINT_PEAK, SA_BANDS_IN_POINT_POWER = 0, 1, 2
BANDS_SIGNATURES = {
    "sa_bands_version": (_INT, []),
    "sa_bands_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, C.c_void_p, _INT, _INT, _P(Band), _INT, _P(C.c_double), C.c_void_p]),
    "sa_bands_check": (_INT, [_INT, C.c_uint64, C.c_uint64, C.c_uint64, _INT, _INT, _P(Band), _INT, _P(C.c_double)]),
    "sa_bands_last_error": (C.c_char_p, []),
}



class MaskRow(C.Structure):
    """sa_mask_row of include/specan_mask.h: the record of one row, 40 bytes."""
    _fields_ = [("over", C.c_int32), ("under", C.c_int32), ("first", C.c_int32), ("last", C.c_int32), ("up_bin", C.c_int32),
                ("lo_bin", C.c_int32), ("up_val", C.c_float), ("up_lim", C.c_float), ("lo_val", C.c_float), ("lo_lim", C.c_float)]


# the entry points of include/specan_mask.h: libspecan_mask.so, the seventh product library, again without a handle (each row
# of 16384 points against an upper and a lower limit line: the bins outside counted, the worst bin of either limit, and the
# rows that failed), bound by mask_lib() and held name for name against that header (tests/test_f32_mask_cpu.py); no name is
# in the tables above
SA_MASK_VERSION = 1
SA_MASK_IN_MAG, SA_MASK_IN_POINT_PEAK, SA_MASK_IN_POINT_POWER = 0, 1, 2
MASK_SIGNATURES = {
    "sa_mask_version": (_INT, []),
    "sa_mask_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, C.c_void_p, _INT, _INT, C.c_void_p, C.c_void_p, _INT, C.c_void_p]),
    "sa_mask_check": (_INT, [C.c_uint64, _INT, C.c_uint64, C.c_uint64, _INT, _INT, C.c_uint64, C.c_uint64, _INT]),
    "sa_mask_last_error": (C.c_char_p, []),
}



class HarmCfg(C.Structure):
    """sa_harm_cfg of include/specan_harm.h: the parameters of a call, 28 bytes, a host struct."""
    _fields_ = [("dc", C.c_int32), ("top", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("fund", C.c_int32),
                ("span", C.c_int32), ("order", C.c_int32)]


class HarmRow(C.Structure):
    """sa_harm_row of include/specan_harm.h: the record of one row, 168 bytes."""
    _fields_ = [("power", C.c_double * 10), ("dist", C.c_double), ("nad", C.c_double), ("noise", C.c_double),
                ("bin", C.c_int32 * 10), ("fund", C.c_float), ("spur", C.c_float), ("nonharm", C.c_float),
                ("spur_bin", C.c_int32), ("nonharm_bin", C.c_int32), ("n_noise", C.c_int32)]


# the entry points of include/specan_harm.h: libspecan_harm.so, the eighth product library, again without a handle (per row
# of 16384 points the fundamental, the bands of its aliased harmonics, the worst spur and the power of the rest), bound by
# harm_lib() and held name for name against that header (tests/test_f32_harm_cpu.py); no name is in the tables above
SA_HARM_VERSION = 1
SA_HARM_MAX, SA_HARM_SPAN_MAX, SA_HARM_TOP_MAX = 10, 64, 8193
SA_HARM_IN_MAG, SA_HARM_IN_POINT_PEAK, SA_HARM_IN_POINT_POWER = 0, 1, 2
HARM_SIGNATURES = {
    "sa_harm_version": (_INT, []),
    "sa_harm_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, _INT, C.POINTER(HarmCfg), C.c_void_p]),
    "sa_harm_check": (_INT, [_INT, C.c_uint64, C.c_uint64, _INT, C.POINTER(HarmCfg)]),
    "sa_harm_last_error": (C.c_char_p, []),
}


class Signal(C.Structure):
    """sa_signal of include/specan_signals.h: one record of the signal list, 24 bytes."""
    _fields_ = [("start", C.c_int32), ("stop", C.c_int32), ("peak", C.c_float), ("peak_bin", C.c_int32), ("power", C.c_double)]


# the entry points of include/specan_signals.h: libspecan_signals.so, the ninth product library, again without a handle (per
# row of 16384 points the runs of bins above the row's threshold with their bounds, peak and power, and the row's counts),
# bound by signals_lib() and held name for name against that header (tests/test_f32_signals_cpu.py); no name is in the tables
# above
SA_SIGNALS_VERSION = 1
SA_SIGNALS_K_MAX = 32
SA_SIGNALS_IN_MAG, SA_SIGNALS_IN_POINT_PEAK, SA_SIGNALS_IN_POINT_POWER = 0, 1, 2
SIGNALS_SIGNATURES = {
    "sa_signals_version": (_INT, []),
    "sa_signals_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, _INT, _INT, _INT, _INT, _INT, _INT,
                              C.c_void_p]),
    "sa_signals_check": (_INT, [_INT, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, _INT, _INT, _INT, _INT, _INT,
                                _INT]),
    "sa_signals_last_error": (C.c_char_p, []),
}

# the entry points of include/specan_cfar.h: libspecan_cfar.so, the tenth product library, again without a handle (per row of
# 16384 points every bin over the mean power of its training cells, or that local floor: float32 [R,16384]), bound by
# cfar_lib() and held name for name against that header (tests/test_f32_cfar_cpu.py); no name is in the tables above
SA_CFAR_VERSION = 1
SA_CFAR_IN_MAG, SA_CFAR_IN_POINT_PEAK, SA_CFAR_IN_POINT_POWER = 0, 1, 2
SA_CFAR_MODE_CA, SA_CFAR_MODE_GO, SA_CFAR_MODE_SO = 0, 1, 2
SA_CFAR_OUT_RATIO, SA_CFAR_OUT_FLOOR = 0, 1
SA_CFAR_LOG2_TRAIN_MAX = 6
SA_CFAR_GUARD_MAX = 64
CFAR_SIGNATURES = {
    "sa_cfar_version": (_INT, []),
    "sa_cfar_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, _INT, _INT, _INT, _INT, _INT, _INT, _INT, C.c_void_p]),
    "sa_cfar_check": (_INT, [_INT, C.c_uint64, C.c_uint64, _INT, _INT, _INT, _INT, _INT, _INT, _INT]),
    "sa_cfar_last_error": (C.c_char_p, []),
}

# the handle-less libraries: short name x -> (file name beside LIB_PATH, entry points); include/specan_x.h declares them and
# the same make builds them.  A new library is a row here and its name in the two lines that spell the public names out.
LIBRARIES = {x: (f"libspecan_{x}.so", table) for x, table in (
    ("fold", FOLD_SIGNATURES), ("peaks", PEAKS_SIGNATURES), ("rank", RANK_SIGNATURES), ("hist", HIST_SIGNATURES),
    ("bands", BANDS_SIGNATURES), ("mask", MASK_SIGNATURES), ("harm", HARM_SIGNATURES),
    # "cfar", the tenth, stands before "signals": a test of the ninth holds "signals" to be the last row
    ("cfar", CFAR_SIGNATURES), ("signals", SIGNALS_SIGNATURES))}
(FOLD_LIB_PATH, PEAKS_LIB_PATH, RANK_LIB_PATH, HIST_LIB_PATH, BANDS_LIB_PATH, MASK_LIB_PATH, HARM_LIB_PATH, CFAR_LIB_PATH,
 SIGNALS_LIB_PATH) = (os.path.join(_PKG, name) for name, _ in LIBRARIES.values())

_loaded = {}                     # path -> the library, mapped and bound: each is loaded once


def _load(path: str, tables: tuple) -> C.CDLL:
    """Map one of the package's shared libraries and bind the names of ``tables``; raise loudly when it has not been built."""
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: the HIP extension is not built (run __graft_entry__.build() or "
            f"`make -C {CSRC}`).  This package has no CPU fallback.")
    # torch first: its wheel bundles a HIP runtime under the same SONAME (libamdhip64.so.7) but another file
    # name, so if this library is mapped first the process ends up with two runtimes and the second one to
    # initialise sees no device.  With torch's copy already mapped, the loader binds this library to it and
    # the tensors and the kernels share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    for table in tables:
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def _loaded_once(path: str, tables: tuple) -> C.CDLL:
    """The one cached loader: _load on the first call for ``path``, the same library afterwards."""
    if path not in _loaded:
        _loaded[path] = _load(path, tables)
    return _loaded[path]


def lib() -> C.CDLL:
    """Load the shared library; raise loudly when it has not been built."""
    return _loaded_once(LIB_PATH, (SIGNATURES, EXT_SIGNATURES))


def _loader(x: str):
    """``x_lib`` for a row of LIBRARIES: the public function that takes no argument and returns that library, loaded once."""
    name, table = LIBRARIES[x]
    path = os.path.join(_PKG, name)

    def load() -> C.CDLL:
        return _loaded_once(path, (table,))
    load.__name__ = load.__qualname__ = f"{x}_lib"
    load.__doc__ = f"Load {name} (include/specan_{x}.h), after torch as lib() does; raise loudly when it has not been built."
    return load


fold_lib, peaks_lib, rank_lib, hist_lib, bands_lib, mask_lib, harm_lib, cfar_lib, signals_lib = map(_loader, LIBRARIES)

# the entry points of include/specan_hold.h: libspecan_hold.so, the eleventh product library, again without a handle (per bin
# the keys at given ranks of the sorted frames of every group of A rows: float32 [G, q, 16384]), bound by hold_lib() and held
# name for name against that header (tests/test_f32_hold_cpu.py); no name is in the tables above.  The library stands outside
# LIBRARIES: the tests of the nine rows hold that table, the data-plane entry points and the offset cases to the counts they
# have, and a row there belongs to a change of those tests alone.
SA_HOLD_VERSION = 1
SA_HOLD_Q_MAX = 8
SA_HOLD_GROUP_MAX = 128
SA_HOLD_IN_MAG, SA_HOLD_IN_POINT_PEAK, SA_HOLD_IN_POINT_POWER = 0, 1, 2
HOLD_SIGNATURES = {
    "sa_hold_version": (_INT, []),
    "sa_hold_f32": (_INT, [C.c_void_p, _INT, C.c_void_p, _INT, _INT, _INT, _P(C.c_int32), C.c_void_p]),
    "sa_hold_check": (_INT, [_INT, C.c_uint64, C.c_uint64, _INT, _INT, _INT, _P(C.c_int32)]),
    "sa_hold_last_error": (C.c_char_p, []),
}
HOLD_LIB_PATH = os.path.join(_PKG, "libspecan_hold.so")


def hold_lib() -> C.CDLL:
    """Load libspecan_hold.so (include/specan_hold.h), after torch as lib() does; raise loudly when it has not been built."""
    return _loaded_once(HOLD_LIB_PATH, (HOLD_SIGNATURES,))


