#!/usr/bin/env python3
"""A/B timing of the cascade kernels behind the integer input forms, which bench.py does not launch: two builds of the
library in one process, alternating rounds, B = 4096, int16 and packed 12-bit samples, the six-section Butterworth of
tests/golden/g2_config1.npz in custom mode:  out 'time' in float32 precision (time_f32_kernel), 'mag_full' and 'time' in
float64 state (iir_f64_kernel).  The first library is the yardstick: the other's median is printed against its min-max.
usage: stage_in_ab.py libspecan_ab_parent.so libspecan_hip.so [--rounds R] [--calls C]   (paths relative to the package
dir; `make -C csrc ab NAME=x` builds libspecan_ab_x.so; GPU)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "fpga_real_time_fft_analyzer_amd")
from fpga_real_time_fft_analyzer_amd.ingest import pack12  # noqa: E402

B, N, ROT = 4096, 16384, 4
KINDS = {"mag_full": 0, "time": 3}


def open_lib(name, sos):
    L = C.CDLL(os.path.join(PKG, name))
    h = C.c_void_p()
    assert L.sa_create(0, C.byref(h)) == 0
    L.sa_load_sos_f64.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.sa_set_filter_mode.argtypes = [C.c_void_p, C.c_uint8]
    L.sa_set_precision.argtypes = [C.c_void_p, C.c_int]
    for f in (L.sa_process_f32_i16, L.sa_process_f32_p12):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert L.sa_load_sos_f64(h, sos.ctypes.data_as(C.POINTER(C.c_double)), len(sos)) == 0
    assert L.sa_set_filter_mode(h, 0xA1) == 0
    return L, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    sos = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "g2_config1.npz"))["sos"], np.float64)
    rng = np.random.default_rng(1)
    # ROT inputs and outputs round-robin, so that a launch streams from HBM and not from the Infinity Cache
    host = [rng.integers(-2048, 2048, size=(B, N)).astype(np.int16) for _ in range(ROT)]
    xs = {"i16": [torch.from_numpy(x).cuda() for x in host], "p12": [torch.from_numpy(pack12(x)).cuda() for x in host]}
    outs = [torch.empty(B, N, device="cuda") for _ in range(ROT)]
    st = torch.cuda.current_stream().cuda_stream
    libs = [(name,) + open_lib(name, sos) for name in a.libs]

    def call(L, h, form, i, kind):
        f = L.sa_process_f32_i16 if form == "i16" else L.sa_process_f32_p12
        rc = f(h, xs[form][i % ROT].data_ptr(), 1.0 / 2048.0, outs[i % ROT].data_ptr(), B, KINDS[kind], st)
        assert rc == 0, rc

    for prec, kind in ((0, "time"), (1, "mag_full"), (1, "time")):
        for form in ("i16", "p12"):
            times, first = {name: [] for name, _, _ in libs}, None
            for rnd in range(a.rounds):
                for name, L, h in (libs if rnd % 2 == 0 else libs[::-1]):       # no build always runs first
                    assert L.sa_set_precision(h, prec) == 0
                    for i in range(3):
                        call(L, h, form, 0, kind)
                    torch.cuda.synchronize()
                    if rnd == 0:                                                # the two builds give the same bits
                        if first is None:
                            first = outs[0].clone()
                        else:
                            assert torch.equal(first, outs[0]), (prec, kind, form)
                    t0 = time.perf_counter()
                    for i in range(a.calls):
                        call(L, h, form, i, kind)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / a.calls * 1e6)
            (n0, _, _), (n1, _, _) = libs
            lo, hi, med = min(times[n0]), max(times[n0]), float(np.median(times[n1]))
            print(f"{'f64' if prec else 'f32'} {kind:8s} {form}: {n0} median {np.median(times[n0]):7.1f} us (min {lo:.1f}, max {hi:.1f})   "
                  f"{n1} median {med:7.1f} us (min {min(times[n1]):.1f}, max {max(times[n1]):.1f})   "
                  f"{'inside' if lo <= med <= hi else 'BELOW (faster than)' if med < lo else 'ABOVE (slower than)'} the first "
                  f"library's min-max; bits equal", flush=True)


if __name__ == "__main__":
    main()
