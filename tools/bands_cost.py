#!/usr/bin/env python3
"""Cost of the band power (include/specan_bands.h; SpectrumChain.band_power and channel_power_f32) on B = 4096 rows.  Every
column is timed between a pair of events on the current stream around the one operation; the columns of a part alternate in
one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the spread of
its columns' own round medians, never against a stored number.
Part 1: the call alone through the C entry point (no allocation between the events) at (nb, nq) = (1, 0), (3, 2), (16, 0) and
        (16, 4) with full-width bands and at (16, 4) with bands of 256 bins, for field 0 on 256 MiB of magnitudes (4096 rows) and
        for field 2 on 256 MiB of records (2048 rows), on three data sets -- "tones": three tones plus noise through filter
        mode 0xB1 ('mag_full', and the records of spectra_f32(group=2)); "wide": exp(uniform +-40); "const": one value --
        against the yardstick of the same run, a device-to-device copy_ of the same input tensor, and against what a caller
        can do on the device today: ``t.double().square()[:, lo:hi].sum(1)`` per band (three bands) and ``cumsum`` +
        ``searchsorted`` per crossing (one band, two fractions; field 0 only).  Every column rotates over three equal inputs
        (768 MiB), so that no call finds its input in the 256 MiB Infinity Cache.
Part 2: channel_power_f32 against process_f32('mag_full'), the call it contains; and with group=4.
Part 3: both with the result copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: bands_cost.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when one
is given: profiles/r22_bands_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
import argparse
import ctypes
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
FULL = [(0, N), (100, 16000), (1, N - 1)]
# name -> (bands, fractions): full-width bands (every tile between the edges is shared), and 16 bands of 256 bins that each
# straddle two tiles
CONFIGS = {
    "b1q0": (FULL[:1], ()),
    "b3q2": (FULL, (0.005, 0.995)),
    "b16q0": ([(j, N - j) for j in range(16)], ()),
    "b16q4": ([(j, N - j) for j in range(16)], (0.005, 0.25, 0.5, 0.995)),
    "n16q4": ([(1000 * j + 100, 1000 * j + 356) for j in range(16)], (0.005, 0.25, 0.5, 0.995)),
}


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

    say(f"tools/bands_cost.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    L = abi.bands_lib()
    stream = torch.cuda.current_stream().cuda_stream
    c_bands = {k: (abi.Band * len(b))(*(abi.Band(lo, hi) for lo, hi in b)) for k, (b, _) in CONFIGS.items()}
    c_fracs = {k: (ctypes.c_double * len(f))(*f) if f else None for k, (_, f) in CONFIGS.items()}
    with SpectrumChain(0) as ch:
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        torch.cuda.synchronize()

        def data_set(name, field):
            """256 MiB of the data set in the layout: float32 [B, N], or records [B / 2, N, 2] whose second float is the point"""
            if name == "tones":
                return mag.clone() if field == 0 else ch.spectra_f32(xd, 2)
            g = torch.Generator(device="cuda").manual_seed(11)
            shape = (B, N) if field == 0 else (B // 2, N, 2)
            if name == "wide":
                return torch.exp(torch.empty(shape, dtype=torch.float32, device="cuda").uniform_(-40.0, 40.0, generator=g))
            return torch.full(shape, 0.37, dtype=torch.float32, device="cuda")

        # part 1: the call alone against the yardsticks, inputs rotating over three tensors
        turn = itertools.count()
        power = torch.empty((B, 16), dtype=torch.float64, device="cuda")
        cross = torch.empty((B, 16, 4), dtype=torch.int32, device="cuda")
        for name in ("tones", "wide", "const"):
            for field in (0, 2):
                t = data_set(name, field)
                torch.cuda.synchronize()
                R = t.shape[0]
                head = np.ascontiguousarray(t[:64].cpu().numpy())
                for k, (bands, fracs) in CONFIGS.items():      # the timed call computes what the mirror says
                    got = ch.band_power(t[:64], bands, fracs, field="power" if field else None)
                    want = frames.bands_of_rows(head, bands, fracs, field="power" if field else None)
                    same = np.array_equal(got[0].cpu().numpy().view(np.uint64), want[0].view(np.uint64)) and (
                        not fracs or np.array_equal(got[1].cpu().numpy(), want[1]))
                    say(f"{name}, field {field}, {k}: the first 64 rows {'equal' if same else 'DIFFER FROM'} frames.bands_of_rows bit for bit")
                srcs = [t] + [t.clone() for _ in range(2)]
                dst = torch.empty_like(t)

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def torch_sums():
                    v = srcs[next(turn) % 3]
                    v = (v if field == 0 else v[..., 1]).double()
                    v = v.square() if field == 0 else v
                    return [v[:, lo:hi].sum(1) for lo, hi in FULL]

                def torch_cross():
                    c = srcs[next(turn) % 3].double().square()[:, 100:16000].cumsum(1)
                    total = c[:, -1:]
                    return torch.searchsorted(c, total * torch.tensor([[0.005, 0.995]], dtype=torch.float64, device="cuda"))

                def call(k):
                    bands, fracs = CONFIGS[k]
                    rc = L.sa_bands_f32(srcs[next(turn) % 3].data_ptr(), field, power.data_ptr(), cross.data_ptr(), R, len(bands),
                                        c_bands[k], len(fracs), c_fracs[k], stream)
                    assert rc == 0, L.sa_bands_last_error()

                calls = {"copy_": copy, "torch3": torch_sums}
                if field == 0:
                    calls["torchq2"] = torch_cross
                for k in CONFIGS:
                    calls[k] = lambda k=k: call(k)
                c = part(f"part 1, {name}, field {field}, {R} rows", list(calls), calls)
                say("          bands / copy_: " + "  ".join(f"{k} {c[k] / c['copy_']:.3f}" for k in CONFIGS)
                    + f"   torch3 / b3q2: {c['torch3'] / c['b3q2']:.1f}"
                    + (f"   torchq2 / b3q2: {c['torchq2'] / c['b3q2']:.1f}" if field == 0 else "")
                    + f"   input bytes / time: copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s  "
                    + "  ".join(f"{k} {t.numel() * 4 / c[k] / 1e6:.2f}" for k in CONFIGS))
                del srcs, dst, t
                torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        acp = frames.channel_bands(4000, 600, 800, 1)
        kw = {"b3q0": dict(bands=acp), "b3q2": dict(bands=acp, fracs=(0.005, 0.995)), "b16q4": dict(bands=CONFIGS["b16q4"][0], fracs=CONFIGS["b16q4"][1]),
              "b3q2 group4": dict(bands=acp, fracs=(0.005, 0.995), group=4)}
        outs = {name: (torch.empty((B // v.get("group", 1), len(v["bands"])), dtype=torch.float64, device="cuda"),
                       torch.empty((B // v.get("group", 1), len(v["bands"]), len(v.get("fracs", ()))), dtype=torch.int32, device="cuda"))
                for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.channel_power_f32(xd, power=outs[name][0], cross=outs[name][1], **v)
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          channel_power / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def power_and_copy(name):
            calls2[name]()
            at = 0
            for o in outs[name]:
                if o.numel():
                    nbytes = o.numel() * o.element_size()
                    host[at:at + nbytes].copy_(o.view(-1).view(torch.uint8), non_blocking=True)
                    at += nbytes

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: power_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / channel_power: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
