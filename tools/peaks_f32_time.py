#!/usr/bin/env python3
"""Cost of the peak table (include/specan_peaks.h; SpectrumChain.find_peaks and peak_table_f32) on chain output of B = 4096
frames, tones plus noise in filter mode 0xB1.  Every column is timed between a pair of events on the current stream around the
one operation; the columns of a part alternate in one process over several rounds (each round: a warm-up call, then a timed
train), and a ratio is read beside the spread of its columns' own round medians, never against a stored number.
Part 1: the find alone through the C entry point (no allocation between the events), for field 0 on the 256 MiB of 'mag_full'
        (4096 rows) and for field 2 on the 256 MiB of spectra_f32(group=2) records (2048 rows), K = 1, 8, 32 and min_sep = 1, 64,
        against a device-to-device copy_ of the same input tensor.  Every column rotates over three equal inputs (768 MiB), so
        that no call finds its input in the 256 MiB Infinity Cache.  Taken twice: at threshold 0 (thousands of candidates per
        row) and at a threshold found here that leaves fewer than 32 in every row.
Part 2: peak_table_f32 against process_f32('mag_full'), the call it contains; and with group=4.
Part 3: both with the result (records and counts) copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: peaks_f32_time.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when one
is given: profiles/r17_peaks_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
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
KS = (1, 8, 32)
SEPS = (1, 64)


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

    rng = np.random.default_rng(7)
    n = np.arange(N)
    D = min(B, 256)                                            # three tones + noise: 256 distinct frames, repeated
    x = sum(amp * np.sin(2 * np.pi * rng.uniform(0.01, 0.45, (D, 1)) * n) for amp in (0.5, 0.2, 0.08)) + 0.05 * rng.standard_normal((D, N))
    xd = torch.from_numpy(x.astype(np.float32)).cuda().repeat((B + D - 1) // D, 1)[:B].contiguous()
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

    say(f"tools/peaks_f32_time.py: B = {B}, filter mode 0xB1, {a.rounds} alternating rounds of {a.calls} timed calls per column; "
        f"us per call, events around the one operation on one stream")
    L = abi.peaks_lib()
    stream = torch.cuda.current_stream().cuda_stream
    with SpectrumChain(0) as ch:
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        rec = ch.spectra_f32(xd, 2)                            # [B / 2, N, 2]: as many bytes as `mag`
        torch.cuda.synchronize()
        inputs = {0: (mag, None), 2: (rec, "power")}
        out = torch.empty((B, 32, 2), dtype=torch.int32, device="cuda")
        count = torch.empty((B,), dtype=torch.int32, device="cuda")

        def low_threshold(t, field):
            """a threshold that leaves fewer than 32 candidates in every row: the largest point / 4, doubled until it does"""
            pts = t if field is None else t[..., 1]
            thr = float(pts.max().item()) / 4.0
            while True:
                c = ch.find_peaks(t, k=1, threshold=thr, field=field)[2]
                if int(c.max().item()) < 32:
                    return thr, int(c.min().item()), int(c.max().item())
                thr *= 2.0

        thr_of = {}
        for code, (t, field) in inputs.items():
            c0 = ch.find_peaks(t, k=1, field=field)[2]
            thr_of[code] = low_threshold(t, field)
            say(f"field {code}: {t.shape[0]} rows, {t.numel() * 4 >> 20} MiB; candidates per row at threshold 0: {int(c0.min().item())}"
                f"..{int(c0.max().item())}; at threshold {thr_of[code][0]:.6g}: {thr_of[code][1]}..{thr_of[code][2]}")
            head = np.ascontiguousarray((t[:64] if field is None else t[:64, :, 1]).cpu().numpy())
            for k, sep, thr in ((32, 64, 0.0), (8, 1, thr_of[code][0])):     # the timed call computes what the mirror says
                got = ch.find_peaks(t[:64], k=k, threshold=thr, min_sep=sep, field=field)
                want = frames.peaks_of_rows(head, k, thr, 0, N, sep)
                same = all(np.array_equal(g.contiguous().cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
                           for g, w in zip(got, want))
                say(f"field {code} K{k} sep{sep} threshold {thr:.6g}: the first 64 rows {'equal' if same else 'DIFFER FROM'} "
                    f"frames.peaks_of_rows bit for bit")
        # part 1: the find alone against a device-to-device copy of the same tensor, inputs rotating over three tensors
        turn = itertools.count()
        c1 = {}
        for code, (t, field) in inputs.items():
            srcs = [t] + [t.clone() for _ in range(2)]
            dsts = [torch.empty_like(t) for _ in range(2)]
            R = t.shape[0]
            for tag, thr in (("threshold 0", 0.0), (f"threshold {thr_of[code][0]:.4g}", thr_of[code][0])):
                def copy():
                    i = next(turn)
                    dsts[i % 2].copy_(srcs[i % 3])

                def find(k, sep, thr=thr):
                    rc = L.sa_peaks_f32(srcs[next(turn) % 3].data_ptr(), code, out.data_ptr(), count.data_ptr(), R, k, thr, 0, N, sep, stream)
                    assert rc == 0, L.sa_peaks_last_error()

                calls = {"copy_": copy}
                for k in KS:
                    for sep in SEPS:
                        calls[f"K{k}/sep{sep}"] = lambda k=k, sep=sep: find(k, sep)
                c = c1[(code, tag)] = part(f"part 1, field {code}, {tag}", list(calls), calls)
                say("          find / copy_: " + "  ".join(f"{k} {c[k] / c['copy_']:.3f}" for k in calls if k != "copy_")
                    + f"   input bytes / time: copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s  "
                    + "  ".join(f"{k} {t.numel() * 4 / c[k] / 1e6:.2f}" for k in calls if k != "copy_"))
            del srcs, dsts
        # part 2: the composed call against the call it contains
        low = thr_of[0][0]
        kw = {"K8/sep1 thr0": dict(k=8), "K8/sep64 thr0": dict(k=8, min_sep=64), "K32/sep64 thr0": dict(k=32, min_sep=64),
              "K8/sep1 thr": dict(k=8, threshold=low), "K8/sep64 group4 thr0": dict(k=8, min_sep=64, group=4)}
        outs = {name: torch.empty((B // v.get("group", 1), v["k"], 2), dtype=torch.int32, device="cuda") for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        res = {}
        for name, v in kw.items():
            def table(name=name, v=v):
                res[name] = ch.peak_table_f32(xd, out=outs[name], **v)
            calls2[name] = table
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          peak_table / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()
        host_count = torch.empty(B, dtype=torch.int32).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def table_and_copy(name):
            calls2[name]()
            o, cnt = outs[name], res[name][2]
            host[:o.numel() * 4].copy_(o.view(-1).view(torch.uint8), non_blocking=True)
            host_count[:cnt.numel()].copy_(cnt, non_blocking=True)

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: table_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / peak_table: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
