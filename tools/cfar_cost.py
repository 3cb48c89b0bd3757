#!/usr/bin/env python3
"""Cost of the CFAR normalisation (include/specan_cfar.h; SpectrumChain.cfar and cfar_f32) on B = 4096 rows.
Every column is timed between a pair of events on the current stream around the one operation; the columns of a part
alternate in one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the
spread of its columns' own round medians, never against a stored number.
Part 1: the call alone through the C entry point (no allocation between the events) at train = 4, 16 and 64 (guard 2, the
        full range, the ratio) in each of the three modes -- for field 0 on 256 MiB of magnitudes (4096 rows) and for field 2
        on 256 MiB of records (2048 rows) of exponentially distributed power on a floor that falls 40 dB across the span --
        against a device-to-device copy_ of the same input tensor in the same run: for magnitudes the call reads and writes
        what the copy does (records: it writes half as much), so the copy is the yardstick; and against what a caller can do
        today in torch on the same tensors for the cell-averaging form at train = 16: two avg_pool1d windows on
        double().square(), their difference and the quotient, which counts the cells beyond the row's ends as zeros among
        2 T and has neither the greatest-of nor the smallest-of form.
        Every column rotates over three equal inputs (768 MiB), so that no call finds its input in the 256 MiB Infinity Cache.
Part 2: cfar_f32 against process_f32('mag_full'), the call it contains; and with group=4.
usage: cfar_cost.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when
one is given: profiles/r26_cfar_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
import argparse
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fpga_real_time_fft_analyzer_amd import abi, frames  # noqa: E402
from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain  # noqa: E402

N = 16384
TRAINS = (4, 16, 64)
MODES = ("ca", "go", "so")
GUARD = 2


def spread(v):
    return f"{min(v):.1f}-{max(v):.1f} ({max(v) / min(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    B = a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]

    def by_events(fn):
        """median us of `fn` over a train of a.calls, each between its own pair of events on the current stream"""
        fn()
        torch.cuda.synchronize()
        for s, e in ev:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        return float(np.median([s.elapsed_time(e) for s, e in ev])) * 1e3

    def part(title, cols, calls):
        med = {k: [] for k in cols}
        for _ in range(a.rounds):
            for k in cols:
                med[k].append(by_events(calls[k]))
        c = {k: float(np.median(med[k])) for k in cols}
        say(f"{title}: " + "  ".join(f"{k} {c[k]:8.1f}" for k in cols))
        say("          round medians: " + "  ".join(f"{k} {spread(med[k])}" for k in cols))
        return c

    say(f"tools/cfar_cost.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    L = abi.cfar_lib()
    stream = torch.cuda.current_stream().cuda_stream
    D = min(B, 256)                                            # 256 distinct rows, repeated
    g = torch.Generator(device="cuda").manual_seed(26)
    floor = 10.0 ** (-4.0 * torch.arange(N, device="cuda") / N)
    power = -torch.log1p(-torch.rand((D, N), device="cuda", generator=g)) * floor       # exponentially distributed
    n = np.arange(N)
    rng = np.random.default_rng(7)
    x = sum(amp * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) for amp in (0.5, 0.2, 0.08)) + 0.05 * rng.standard_normal((D, N))
    xd = torch.from_numpy(x.astype(np.float32)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
    configs = {f"{m}{T}": (m, T) for T in TRAINS for m in MODES}
    with SpectrumChain(0) as ch:
        # part 1: the call alone against the copy, inputs rotating over three tensors
        turn = itertools.count()
        for field in (0, 2):
            R = B if field == 0 else B // 2
            rows = (power.sqrt() if field == 0 else power).repeat((R + D - 1) // D, 1)[:R].contiguous()
            if field == 0:
                t = rows
            else:
                t = torch.zeros((R, N, 2), dtype=torch.float32, device="cuda")
                t[..., 1] = rows
            fname = "power" if field else None
            head = np.ascontiguousarray(t[:16].cpu().numpy())
            for c, (m, T) in configs.items():                  # the timed call computes what the mirror says
                got = ch.cfar(t[:16], T, GUARD, m, field=fname).view(torch.int32).cpu().numpy()
                want = frames.cfar_of_rows(head, T, GUARD, m, field=fname).view(np.int32)
                say(f"field {field}, {c}: the first 16 rows {'equal' if np.array_equal(got, want) else 'DIFFER FROM'} "
                    f"frames.cfar_of_rows bit for bit")
            srcs = [t] + [t.clone() for _ in range(2)]
            dst = torch.empty_like(t)
            out = torch.empty((R, N), dtype=torch.float32, device="cuda")

            def copy():
                dst.copy_(srcs[next(turn) % 3])

            def torch_ca():
                """the cell-averaging ratio at train 16 in torch: the window of 2 (G + T) + 1 cells less that of 2 G + 1"""
                src = srcs[next(turn) % 3]
                p = (src.double().square() if field == 0 else src[..., 1].double())[:, None, :]
                wide = torch.nn.functional.avg_pool1d(p, 2 * (GUARD + 16) + 1, 1, GUARD + 16) * (2 * (GUARD + 16) + 1)
                inner = torch.nn.functional.avg_pool1d(p, 2 * GUARD + 1, 1, GUARD) * (2 * GUARD + 1)
                return (p * 32.0 / (wide - inner))[:, 0, :].float()

            def call(c):
                m, T = configs[c]
                rc = L.sa_cfar_f32(srcs[next(turn) % 3].data_ptr(), field, out.data_ptr(), R, T.bit_length() - 1, GUARD, MODES.index(m), 0,
                                   0, N, stream)
                assert rc == 0, L.sa_cfar_last_error()

            calls = {"copy_": copy, "torch": torch_ca}
            for c in configs:
                calls[c] = lambda c=c: call(c)
            m = part(f"part 1, field {field}, {R} rows", list(calls), calls)
            say("          cfar / copy_: " + "  ".join(f"{c} {m[c] / m['copy_']:.3f}" for c in configs)
                + f"   torch / ca16: {m['torch'] / m['ca16']:.1f}"
                + f"   input bytes / time: copy_ {t.numel() * 4 / m['copy_'] / 1e6:.2f} TB/s  "
                + "  ".join(f"{c} {t.numel() * 4 / m[c] / 1e6:.2f}" for c in configs))
            del srcs, dst, t, out
            torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        torch.cuda.synchronize()
        kw = {"ca16": dict(train=16), "go64": dict(train=64, mode="go"), "ca16 group4": dict(train=16, group=4)}
        outs = {name: torch.empty((B // v.get("group", 1), N), dtype=torch.float32, device="cuda") for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.cfar_f32(xd, guard=GUARD, out=outs[name], **v)
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          cfar_f32 / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
