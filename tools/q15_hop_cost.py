#!/usr/bin/env python3
"""Kernel cost of frames cut on the device from one sample stream (SA_Q15_HOP_KIND; process_q15(x, hop=...)) against the
frame call on host-cut copies of the same frames, at B = 4096: device time per call from the launch-timing ring
(sa_set_profiling), one process, the two calls alternating over several rounds (each round: warm-up calls, then a timed
train).  The copies are made once, on the device, by the gather ingest.FrameCutter(hop) makes on the host; the outputs of
the two calls are compared once per row (they must be equal).  Modes 0xB1 (stage 0 of the FFT reads the stream), 0x00 and
0xA2 (the cascades' staging waves do), kinds 'iq' and 'marker', int16 and packed samples, hop = N/2 and N/4.  The frame
call is the reference of its own run -- its kernels are untouched by the hop kernels' existence: compare within a line, never
against a stored number, and read a ratio beside the spread of the frame column's own round medians.
usage: q15_hop_cost.py [--rounds R] [--calls C] [--batch B]   (GPU)"""
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
    print(f"B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per form; us per call, device time "
          f"(launch-timing ring); 'frames': the plain call on [B,16384] copies, 'hop': the call on the stream")
    with SpectrumChain(0) as ch:
        ch.load_sos_q14(sos14)
        ch.reserve(B)
        for hop in (N // 2, N // 4):
            n = (B - 1) * hop + N
            # a slow chirp + noise in the ADC's range, quantised to 12 bits
            t = np.arange(n, dtype=np.float64)
            s = 1500.0 * np.sin(2 * np.pi * (0.01 + 0.2 * t / n) * t) + 200.0 * rng.standard_normal(n)
            si = np.clip(np.rint(s), -2048, 2047).astype(np.int16)
            for form, host, row in (("int16", si, N), ("p12", pack12(si), 3 * N // 2)):
                stream = torch.from_numpy(host).cuda()
                frames = stream.unfold(0, row, row * hop // N).contiguous()         # FrameCutter's gather, on the device
                assert frames.shape == (B, row)
                d = {"frames": (frames, None), "hop": (stream, hop)}
                print(f"hop {hop} {form}: stream {stream.numel() * stream.element_size() / 2**20:.0f} MiB, "
                      f"frames {frames.numel() * frames.element_size() / 2**20:.0f} MiB")
                for mode in (0xB1, 0x00, 0xA2):
                    for kind in ("iq", "marker"):
                        ch.set_filter_mode(mode)
                        outs = {k: ch.process_q15(x, out_kind=kind, hop=h) for k, (x, h) in d.items()}
                        torch.cuda.synchronize()
                        equal = torch.equal(outs["frames"], outs["hop"])
                        ch.set_profiling(a.calls)
                        med = {"frames": [], "hop": []}
                        for _ in range(a.rounds):
                            for k, (x, h) in d.items():
                                for _ in range(2):
                                    ch.process_q15(x, out=outs[k], out_kind=kind, hop=h)
                                torch.cuda.synchronize()
                                for _ in range(a.calls):
                                    ch.process_q15(x, out=outs[k], out_kind=kind, hop=h)
                                ms = ch.profile_read(a.calls)
                                assert len(ms) == a.calls
                                med[k].append(float(np.median(ms)) * 1e3)
                        ch.set_profiling(0)
                        fr, hp = float(np.median(med["frames"])), float(np.median(med["hop"]))
                        lo, hi = min(med["frames"]), max(med["frames"])
                        print(f"  mode 0x{mode:02X} {kind:6s}: frames {fr:7.1f} us  hop {hp:7.1f} us  hop/frames {hp / fr:.3f}   "
                              f"round medians frames {lo:.1f}-{hi:.1f} (max/min {hi / lo:.3f}), hop {min(med['hop']):.1f}-"
                              f"{max(med['hop']):.1f}   outputs equal: {equal}", flush=True)
                        del outs
                del stream, frames, d
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
