#!/usr/bin/env python3
"""Cost of the harmonic analysis (include/specan_harm.h; SpectrumChain.harmonics and harmonics_f32) on B = 4096 rows.
Every column is timed between a pair of events on the current stream around the one operation; the columns of a part
alternate in one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the
spread of its columns' own round medians, never against a stored number.
Part 1: the call alone through the C entry point (no allocation between the events) at (order, span) = (1, 3), (5, 3) and
        (10, 64) -- for field 0 on 256 MiB of magnitudes (4096 rows) and for field 2 on 256 MiB of records (2048 rows), on
        three data sets -- "tones": three tones plus noise through filter mode 0xB1 ('mag_full', and the records of
        spectra_f32(group=2)); "wide": exp(uniform +-40), a fundamental of its own in nearly every row; "const": one value, the
        fundamental of every row at `lo` -- against the yardstick of the same run, a device-to-device copy_ of the same input
        tensor, against the 16-band sa_bands_f32 call without crossings on the same input ("band16"), and against what a caller
        can do today: "today" is the argmax of every row copied to the host, then per distinct fundamental one band_power call
        (the band of the fundamental and of harmonics 2..5) on the rows that have it -- the five powers and nothing else of the
        record; "torch" is the record's content composed of torch calls in float64 (not bit-exact: torch sums in another order).
        Every column rotates over three equal inputs (768 MiB), so that no call finds its input in the 256 MiB Infinity Cache.
Part 2: harmonics_f32 against process_f32('mag_full'), the call it contains; and with group=4.
Part 3: both with the records copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: harm_cost.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when one
is given: profiles/r24_harm_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
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
TOP = 8193
CONFIGS = {"o1s3": (1, 3), "o5s3": (5, 3), "o10s64": (10, 64)}            # name -> (order, span)


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

    say(f"tools/harm_cost.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    L, LB = abi.harm_lib(), abi.bands_lib()
    stream = torch.cuda.current_stream().cuda_stream
    sixteen = (abi.Band * 16)(*(abi.Band(512 * j, 512 * j + 512) for j in range(16)))      # bins 0..8191 in 16 bands
    cfgs = {k: abi.HarmCfg(span + 1, TOP, span + 1, TOP, -1, span, order) for k, (order, span) in CONFIGS.items()}
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
        power16 = torch.empty((B, 16), dtype=torch.float64, device="cuda")
        rows_out = torch.empty((B, 42), dtype=torch.int32, device="cuda")
        offs = torch.arange(-3, 4, device="cuda")
        for name in ("tones", "wide", "const"):
            for field in (0, 2):
                t = data_set(name, field)
                torch.cuda.synchronize()
                R = t.shape[0]
                fname = "power" if field else None
                head = np.ascontiguousarray(t[:64].cpu().numpy())
                for k, (order, span) in CONFIGS.items():         # the timed call computes what the mirror says
                    o = torch.zeros((64, 42), dtype=torch.int32, device="cuda")
                    ch.harmonics(t[:64], order=order, span=span, field=fname, out=o)
                    got = o.cpu().numpy().view(frames.HARM_ROW)[:, 0]
                    want = frames.harm_of_rows(head, order=order, span=span, field=fname)
                    same = all(np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(want[f]).view(np.uint8))
                               for f in frames.HARM_ROW.names)
                    say(f"{name}, field {field}, {k}: the first 64 rows {'equal' if same else 'DIFFER FROM'} frames.harm_of_rows bit for "
                        f"bit; distinct fundamentals {len(set(want['bin'][:, 0].tolist()))}")
                srcs = [t] + [t.clone() for _ in range(2)]
                dst = torch.empty_like(t)

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def band16():
                    rc = LB.sa_bands_f32(srcs[next(turn) % 3].data_ptr(), field, power16.data_ptr(), None, R, 16, sixteen, 0, None, stream)
                    assert rc == 0, LB.sa_bands_last_error()

                def today():
                    """order 5, span 3: the fundamentals to the host, then band_power per distinct fundamental"""
                    src = srcs[next(turn) % 3]
                    v = src if field == 0 else src[..., 1]
                    k1 = (4 + v[:, 4:TOP].abs().argmax(1)).cpu()
                    out = []
                    for k in torch.unique(k1).tolist():
                        bins = frames.harm_alias_bins(k, 5).tolist()
                        bands = [(max(b - 3, 4), min(b + 4, TOP)) for b in bins]
                        rows = torch.nonzero(k1 == k).flatten().cuda()
                        out.append(ch.band_power(src.index_select(0, rows), [b for b in bands if b[0] < b[1]], field=fname)[0])
                    return out

                def torch_harm():
                    """order 5, span 3, in torch: the five band powers, dist, nad, noise, the spur and the non-harmonic spur"""
                    src = srcs[next(turn) % 3]
                    v = (src if field == 0 else src[..., 1])[:, :TOP].abs()
                    p = v.double() if field else v.double().square()
                    k1 = 4 + v[:, 4:].argmax(1)
                    m = (k1[:, None] * torch.arange(1, 6, device="cuda")) % N
                    kh = torch.where(m <= N // 2, m, N - m)
                    idx = (kh[:, :, None] + offs).clamp_(0, TOP - 1)                      # [R, 5, 7]
                    member = torch.zeros(p.shape, dtype=torch.int8, device="cuda")
                    member.scatter_(1, idx[:, 1:].reshape(R, -1), 1)
                    member.scatter_(1, idx[:, 0], 2)
                    member[:, :4] = 2
                    powers = torch.gather(p, 1, idx.reshape(R, -1)).view(R, 5, 7).sum(2)
                    rest = torch.where(member < 2, p, 0.0)
                    noise = torch.where(member == 0, p, 0.0)
                    spur = torch.where(member < 2, v, -1.0).max(1)
                    other = torch.where(member == 0, v, -1.0).max(1)
                    return powers, rest.sum(1), noise.sum(1), spur, other

                def call(k):
                    rc = L.sa_harm_f32(srcs[next(turn) % 3].data_ptr(), field, rows_out.data_ptr(), R, ctypes.byref(cfgs[k]), stream)
                    assert rc == 0, L.sa_harm_last_error()

                calls = {"copy_": copy, "band16": band16, "today": today, "torch": torch_harm}
                for k in CONFIGS:
                    calls[k] = lambda k=k: call(k)
                c = part(f"part 1, {name}, field {field}, {R} rows", list(calls), calls)
                say("          harm / copy_: " + "  ".join(f"{k} {c[k] / c['copy_']:.3f}" for k in CONFIGS)
                    + f"   band16 / copy_: {c['band16'] / c['copy_']:.3f}"
                    + "   harm / band16: " + "  ".join(f"{k} {c[k] / c['band16']:.3f}" for k in CONFIGS)
                    + f"   today / o5s3: {c['today'] / c['o5s3']:.1f}   torch / o5s3: {c['torch'] / c['o5s3']:.1f}"
                    + f"   claimed input bytes / time: copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s  "
                    + "  ".join(f"{k} {t.numel() * 4 / c[k] / 1e6:.2f}" for k in CONFIGS))
                del srcs, dst, t
                torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        kw = {"o1s3": dict(order=1, span=3), "o5s3": dict(order=5, span=3), "o10s64": dict(order=10, span=64),
              "o5s3 group4": dict(order=5, span=3, group=4)}
        outs = {name: torch.empty((B // v.get("group", 1), 42), dtype=torch.int32, device="cuda") for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.harmonics_f32(xd, out=outs[name], **v)
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          harmonics_f32 / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def harm_and_copy(name):
            calls2[name]()
            o = outs[name]
            host[:o.numel() * 4].copy_(o.view(-1).view(torch.uint8), non_blocking=True)

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: harm_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / harmonics_f32: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
