#!/usr/bin/env python3
"""Cost of the spectral mask test (include/specan_mask.h; SpectrumChain.mask_test and mask_trigger_f32) on B = 4096 rows.
Every column is timed between a pair of events on the current stream around the one operation; the columns of a part
alternate in one process over several rounds (each round: a warm-up call, then a timed train), and a ratio is read beside the
spread of its columns' own round medians, never against a stored number.
Part 1: the call alone through the C entry point (no allocation between the events) -- upper limit only ("u"), both limits
        ("ul"), both with the summary ("u+s", "ul+s"), both over a range of 1024 bins ("ul1k") -- for field 0 on 256 MiB of
        magnitudes (4096 rows) and for field 2 on 256 MiB of records (2048 rows), on three data sets -- "tones": three tones
        plus noise through filter mode 0xB1 ('mag_full', and the records of spectra_f32(group=2)) against the envelope of the
        first 64 rows; "wide": exp(uniform +-40) against the same kind of envelope; "violate": one value between a lower limit
        above it and an upper limit below it, so that every bin of every row counts twice -- against the yardstick of the same
        run, a device-to-device copy_ of the same input tensor, against the one-band sa_bands_f32 call on the same input
        ("band1"), and against what a caller can do on the device today: compare and count per limit, the float32 quotient and
        its argmax ("torch").  Every column rotates over three equal inputs (768 MiB), so that no call finds its input in the
        256 MiB Infinity Cache.
Part 2: mask_trigger_f32 against process_f32('mag_full'), the call it contains; and with group=4.
Part 3: both with the result copied to pinned host memory behind the call, against 'mag_full' + its copy.
usage: mask_cost.py [--rounds R] [--calls C] [--batch B] [--out FILE]   (GPU; prints its lines, and writes them to FILE when one
is given: profiles/r23_mask_f32.txt holds a run's lines between sections written by hand, so it is no default)"""
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
NARROW = (4000, 5024)
# name -> (upper given, lower given, summary given, range)
CONFIGS = {
    "u": (True, False, False, (0, N)),
    "ul": (True, True, False, (0, N)),
    "u+s": (True, False, True, (0, N)),
    "ul+s": (True, True, True, (0, N)),
    "ul1k": (True, True, False, NARROW),
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

    say(f"tools/mask_cost.py: B = {B}, {a.rounds} alternating rounds of {a.calls} timed calls per column; us per call, events "
        f"around the one operation on one stream")
    L, LB = abi.mask_lib(), abi.bands_lib()
    stream = torch.cuda.current_stream().cuda_stream
    one_band = (abi.Band * 1)(abi.Band(0, N))
    with SpectrumChain(0) as ch:
        ch.set_filter_mode(0xB1)
        mag = ch.process_f32(xd, out_kind="mag_full")
        torch.cuda.synchronize()

        def data_set(name, field):
            """256 MiB of the data set in the layout -- float32 [B, N], or records [B / 2, N, 2] whose second float is the point
            -- and its limits, float32 [N] on the device"""
            if name == "tones":
                t = mag.clone() if field == 0 else ch.spectra_f32(xd, 2)
            else:
                g = torch.Generator(device="cuda").manual_seed(11)
                shape = (B, N) if field == 0 else (B // 2, N, 2)
                if name == "wide":
                    t = torch.exp(torch.empty(shape, dtype=torch.float32, device="cuda").uniform_(-40.0, 40.0, generator=g))
                else:
                    t = torch.full(shape, 0.37, dtype=torch.float32, device="cuda")
            if name == "violate":
                return t, torch.full((N,), 0.25, dtype=torch.float32, device="cuda"), torch.full((N,), 0.5, dtype=torch.float32, device="cuda")
            pts = t[:64] if field == 0 else t[:64, :, 1]        # the envelope of the first rows: later rows leave it here and there
            return t, pts.amax(0).contiguous(), (pts.amin(0) * 0.5).contiguous()

        # part 1: the call alone against the yardsticks, inputs rotating over three tensors
        turn = itertools.count()
        rows_out = torch.empty((B, 10), dtype=torch.int32, device="cuda")
        summary = torch.empty((4,), dtype=torch.int32, device="cuda")
        power = torch.empty((B,), dtype=torch.float64, device="cuda")
        for name in ("tones", "wide", "violate"):
            for field in (0, 2):
                t, up, low = data_set(name, field)
                torch.cuda.synchronize()
                R = t.shape[0]
                head = np.ascontiguousarray(t[:64].cpu().numpy())
                h_up, h_low = up.cpu().numpy(), low.cpu().numpy()
                for k, (u, l, s, (lo, hi)) in CONFIGS.items():    # the timed call computes what the mirror says
                    got = ch.mask_test(t[:64], up if u else None, low if l else None, lo, hi, field="power" if field else None, summary=s)
                    want, want_s = frames.mask_of_rows(head, h_up if u else None, h_low if l else None, lo, hi, field="power" if field else None)
                    rec = torch.cat([got[0], got[1].view(torch.int32)], dim=1).contiguous().cpu().numpy().view(frames.MASK_ROW)[:, 0]
                    same = rec.tobytes() == want.tobytes() and (not s or got[2].cpu().numpy().tolist() == want_s.tolist())
                    say(f"{name}, field {field}, {k}: the first 64 rows {'equal' if same else 'DIFFER FROM'} frames.mask_of_rows bit for bit; "
                        f"rows over {int((want['over'] > 0).sum())}, under {int((want['under'] > 0).sum())}, bins over {int(want['over'].sum())}")
                srcs = [t] + [t.clone() for _ in range(2)]
                dst = torch.empty_like(t)

                def copy():
                    dst.copy_(srcs[next(turn) % 3])

                def band1():
                    rc = LB.sa_bands_f32(srcs[next(turn) % 3].data_ptr(), field, power.data_ptr(), None, R, 1, one_band, 0, None, stream)
                    assert rc == 0, LB.sa_bands_last_error()

                def torch_mask():
                    v = srcs[next(turn) % 3]
                    v = (v if field == 0 else v[..., 1]).abs()
                    return (v > up).sum(1), (v < low).sum(1), (v / up).argmax(1), (v / low).argmin(1)

                def call(k):
                    u, l, s, (lo, hi) = CONFIGS[k]
                    rc = L.sa_mask_f32(srcs[next(turn) % 3].data_ptr(), field, up.data_ptr() if u else None, low.data_ptr() if l else None,
                                       lo, hi, rows_out.data_ptr(), summary.data_ptr() if s else None, R, stream)
                    assert rc == 0, L.sa_mask_last_error()

                calls = {"copy_": copy, "band1": band1, "torch": torch_mask}
                for k in CONFIGS:
                    calls[k] = lambda k=k: call(k)
                c = part(f"part 1, {name}, field {field}, {R} rows", list(calls), calls)
                say("          mask / copy_: " + "  ".join(f"{k} {c[k] / c['copy_']:.3f}" for k in CONFIGS)
                    + "   mask / band1: " + "  ".join(f"{k} {c[k] / c['band1']:.3f}" for k in CONFIGS)
                    + f"   torch / ul: {c['torch'] / c['ul']:.1f}"
                    + f"   input bytes / time: copy_ {t.numel() * 4 / c['copy_'] / 1e6:.2f} TB/s  band1 {t.numel() * 4 / c['band1'] / 1e6:.2f}  "
                    + "  ".join(f"{k} {t.numel() * 4 / c[k] / 1e6:.2f}" for k in CONFIGS if k != "ul1k"))
                del srcs, dst, t
                torch.cuda.empty_cache()
        # part 2: the composed call against the call it contains
        up = mag[:64].amax(0).contiguous()
        low = (mag[:64].amin(0) * 0.5).contiguous()
        rec4 = ch.spectra_f32(xd[:256], 4)[..., 1]
        up4 = rec4.amax(0).contiguous()
        kw = {"u": dict(upper=up), "ul": dict(upper=up, lower=low), "ul1k": dict(upper=up, lower=low, lo=NARROW[0], hi=NARROW[1]),
              "u group4": dict(upper=up4, group=4)}
        outs = {name: (torch.empty((B // v.get("group", 1), 10), dtype=torch.int32, device="cuda"),
                       torch.empty((4,), dtype=torch.int32, device="cuda")) for name, v in kw.items()}
        calls2 = {"mag_full": lambda: ch.process_f32(xd, out=mag, out_kind="mag_full")}
        for name, v in kw.items():
            calls2[name] = lambda name=name, v=v: ch.mask_trigger_f32(xd, out=outs[name][0], summary=outs[name][1], **v)
        c2 = part("part 2, on the device", list(calls2), calls2)
        say("          mask_trigger / mag_full: " + "  ".join(f"{k} {c2[k] / c2['mag_full']:.3f}" for k in kw))
        # part 3: with the result copied to pinned host memory behind each call
        host = torch.empty(mag.numel() * 4, dtype=torch.uint8).pin_memory()

        def mag_and_copy():
            calls2["mag_full"]()
            host.copy_(mag.view(-1).view(torch.uint8), non_blocking=True)

        def trigger_and_copy(name):
            calls2[name]()
            at = 0
            for o in outs[name]:
                nbytes = o.numel() * o.element_size()
                host[at:at + nbytes].copy_(o.view(-1).view(torch.uint8), non_blocking=True)
                at += nbytes

        calls3 = {"mag_full": mag_and_copy}
        for name in kw:
            calls3[name] = lambda name=name: trigger_and_copy(name)
        c3 = part("part 3, call + copy  ", list(calls3), calls3)
        say("          mag_full / mask_trigger: " + "  ".join(f"{k} {c3['mag_full'] / c3[k]:.2f}" for k in kw))
    if a.out is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
