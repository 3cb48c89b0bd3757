#!/usr/bin/env python3
"""Cost of the float64-state precision at B = 4096: microseconds per sa_process_f32 call in both precisions, in one
process, alternating rounds (each round: warm-up, then a timed train of calls on the current stream), for the headline
12th-order Butterworth (custom mode) and the RTL default taps; plus the per-kernel device times of one f64 call from
the launch-timing ring.  usage: f64_cost.py [--rounds R] [--calls C]   (GPU)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=40)
    a = ap.parse_args()
    B, N = 4096, 16384
    sos = np.load(os.path.join(ROOT, "tests", "golden", "g2_config1.npz"))["sos"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(B, N, generator=gen, device="cuda") for _ in range(2)]
    outs = [torch.empty(B, N, device="cuda") for _ in range(2)]
    with SpectrumChain(0) as ch:
        ch.load_sos(sos)
        ch.reserve(B)
        for mode, name in ((0xA1, "custom: 12th-order Butterworth (6 sections)"), (0x00, "default: RTL taps (6 sections)")):
            ch.set_filter_mode(mode)
            for kind in ("mag_full", "time"):
                times = {"f32": [], "f64": []}
                for _ in range(a.rounds):
                    for prec in ("f32", "f64"):
                        ch.set_precision(prec)
                        for i in range(3):
                            ch.process_f32(xs[i % 2], out=outs[i % 2], out_kind=kind)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for i in range(a.calls):
                            ch.process_f32(xs[i % 2], out=outs[i % 2], out_kind=kind)
                        torch.cuda.synchronize()
                        times[prec].append((time.perf_counter() - t0) / a.calls * 1e6)
                f32, f64 = np.median(times["f32"]), np.median(times["f64"])
                print(f"{name}, out {kind}: f32 {f32:7.1f} us  f64 {f64:7.1f} us per {B}-frame call  (x{f64 / f32:.2f}; "
                      f"medians of {a.rounds} alternating rounds of {a.calls} calls; spread f32 "
                      f"{min(times['f32']):.1f}-{max(times['f32']):.1f}, f64 {min(times['f64']):.1f}-{max(times['f64']):.1f})")
        # device time of a whole f64 call (both kernels) and of the cascade kernel alone (SA_OUT_TIME) from the ring
        ch.set_filter_mode(0xA1)
        ch.set_precision("f64")
        ch.set_profiling(16)
        for i in range(16):
            ch.process_f32(xs[i % 2], out=outs[i % 2])
        call = float(np.median(ch.profile_read(16))) * 1e3
        for i in range(16):
            ch.process_f32(xs[i % 2], out=outs[i % 2], out_kind="time")
        casc = float(np.median(ch.profile_read(16))) * 1e3
        ch.set_profiling(0)
        print(f"launch-timing ring, f64, custom Butterworth, B = {B}: whole call (cascade + FFT) {call:.1f} us, "
              f"cascade kernel alone (out 'time') {casc:.1f} us")


if __name__ == "__main__":
    main()
