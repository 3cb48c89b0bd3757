#!/usr/bin/env python3
"""Kernel cost of the integer chain's packed 12-bit input (sa_process_q15_p12) against its int16 input
(sa_process_q15_out) at B = 4096: device time per call from the launch-timing ring (sa_set_profiling), one process, the
two inputs alternating over several rounds (each round: warm-up calls, then a timed train).  The same samples in both
forms; the outputs of the two calls are compared once per row (they must be equal).  Modes 0xB1 (the unpack sits in
stage 0 of the FFT), 0x00 and 0xA2 (it sits in the cascades' staging waves), kinds 'iq' and 'marker'.  The int16 figure
is the reference of its own run: compare within a line, never against a stored number, and read a ratio beside the
spread of the int16 column's own round medians.  The float chain's counterpart is tools/p12_cost.py.
usage: q15_p12_cost.py [--rounds R] [--calls C] [--batch B]   (GPU)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402
from fpga_real_time_fft_analyzer_amd.ingest import pack12  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    B, N = a.batch, 16384
    from scipy import signal
    # six Q2.14 sections that pass signal: second-order Butterworth low-passes of unity DC gain
    sos14 = np.rint(16384.0 * np.concatenate([signal.butter(2, wc, output="sos") for wc in (0.35, 0.45, 0.55, 0.65, 0.75, 0.85)]))
    sos14 = sos14.astype(np.int16)
    rng = np.random.default_rng(5)
    n = np.arange(N)
    # tones + noise in the ADC's range, quantised to 12 bits: 256 distinct frames, repeated up to the batch
    D = min(B, 256)
    x = 1500.0 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) + 200.0 * rng.standard_normal((D, N))
    xi = np.clip(np.rint(x), -2048, 2047).astype(np.int16)
    reps = (B + D - 1) // D
    d = {"i16": torch.from_numpy(xi).cuda().repeat(reps, 1)[:B].contiguous(),
         "p12": torch.from_numpy(pack12(xi)).cuda().repeat(reps, 1)[:B].contiguous()}
    print(f"B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per input; us per call, device time "
          f"(launch-timing ring); input bytes per frame: int16 32768, p12 24576")
    with SpectrumChain(0) as ch:
        ch.load_sos_q14(sos14)
        ch.reserve(B)
        for mode in (0xB1, 0x00, 0xA2):
            for kind in ("iq", "marker"):
                ch.set_filter_mode(mode)
                outs = {k: ch.process_q15(v, out_kind=kind) for k, v in d.items()}
                torch.cuda.synchronize()
                equal = torch.equal(outs["i16"], outs["p12"])
                ch.set_profiling(a.calls)
                med = {"i16": [], "p12": []}
                for _ in range(a.rounds):
                    for k in ("i16", "p12"):
                        for _ in range(2):
                            ch.process_q15(d[k], out=outs[k], out_kind=kind)
                        torch.cuda.synchronize()
                        for _ in range(a.calls):
                            ch.process_q15(d[k], out=outs[k], out_kind=kind)
                        ms = ch.profile_read(a.calls)
                        assert len(ms) == a.calls
                        med[k].append(float(np.median(ms)) * 1e3)
                ch.set_profiling(0)
                i16, p12 = float(np.median(med["i16"])), float(np.median(med["p12"]))
                lo, hi = min(med["i16"]), max(med["i16"])
                print(f"mode 0x{mode:02X} {kind:6s}: int16 {i16:7.1f} us  p12 {p12:7.1f} us  p12/int16 {p12 / i16:.3f}   "
                      f"round medians int16 {lo:.1f}-{hi:.1f} (max/min {hi / lo:.3f}), p12 {min(med['p12']):.1f}-{max(med['p12']):.1f}"
                      f"   outputs equal: {equal}", flush=True)


if __name__ == "__main__":
    main()
