#!/usr/bin/env python3
"""The randomised parity sweep of tests/fuzz_parity.py with the handle in the float64-state precision
(SpectrumChain.set_precision("f64")): seeds 7, 11 and 23 x 1500 designs by default.  Prints, per seed and in total, the
worst max-norm error of the spectrum against the float64 oracle and the count above 1e-5, next to the sequential
float32 figures of the same designs.  usage: fuzz_f64.py [SEED ...] [--cases N]   (GPU)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fuzz_parity  # noqa: E402
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seeds", nargs="*", type=int, default=[7, 11, 23])
    ap.add_argument("--cases", type=int, default=1500)
    a = ap.parse_args()
    total = over_total = seq_total = 0
    worst_all = 0.0
    with SpectrumChain(0) as ch:
        ch.set_precision("f64")
        for seed in a.seeds:
            res = fuzz_parity.sweep(ch, seed, a.cases)
            over = sorted((r for r in res if not r[0] <= 1e-5), reverse=True)
            seq = sum(1 for r in res if r[2] > 1e-5)
            worst = max(r[0] for r in res)
            print(f"== seed {seed}: {len(res)} designs, worst spectrum err {worst:.2e}, {len(over)} above 1e-5 "
                  f"(a sequential float32 evaluation: {seq} above 1e-5)")
            for err, att, seq_err, label in sorted(res, reverse=True)[:5]:
                print(f"   err {err:.2e}  output/input peak {att:.1e}  sequential-f32 {seq_err:.2e}  {label}")
            total += len(res)
            over_total += len(over)
            seq_total += seq
            worst_all = max(worst_all, worst)
    print(f"precision f64: {over_total} of {total} designs above 1e-5, worst {worst_all:.2e} "
          f"(sequential float32: {seq_total} above 1e-5)")
    return 1 if over_total else 0


if __name__ == "__main__":
    sys.exit(main())
