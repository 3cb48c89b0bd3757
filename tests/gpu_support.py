"""Shared by the GPU test modules (a plain module, like structured_cases.py): the fixtures every one of them asks for,
imported by name into the module that uses them, and the helpers that were the same in two or more of them."""
import copy

import numpy as np
import pytest

import drawn_cases as dc
from conftest import N
from native import Lds, gpu_helper


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lds_fill(tmp_path_factory, torch_mod):
    """tests/hip/lds_fill.hip, built and bound once per module that asks for it: lds_fill(word) writes `word` to all of the
    LDS of every CU, on the current stream."""
    return Lds(gpu_helper(tmp_path_factory.mktemp("lds_fill"), "lds_fill"), torch_mod).fill


@pytest.fixture()
def ch(chain_cls):
    c = chain_cls(0)
    yield c
    c.close()


def to_device(torch_mod, a):
    a = np.ascontiguousarray(a)
    return torch_mod.from_numpy(a if a.flags.writeable else a.copy()).cuda()       # a shared read-only batch is copied


COMPOSED = {"fold": "spectra_f32", "peaks": "peak_table_f32", "rank": "noise_floor_f32", "hist": "persistence_f32",
            "bands": "channel_power_f32", "mask": "mask_trigger_f32", "harm": "harmonics_f32", "signals": "signals_f32",
            "cfar": "cfar_f32"}


class ReductionCall:
    """One call of a reduction library's method (drawn_cases.METHODS), prepared so that making it is nothing but the method
    call: the input resident, the arguments objects of its own (a limit line or a threshold per row on the device, the rest
    copied) and an output of 0xFF bytes for every ``out=`` argument.  ``composed``: the arguments of the composed call that
    stands for the plain call with ``kw``, ``x`` then being the frames."""

    def __init__(self, torch, name, x, field, kw, composed=None):
        self.name, self.x, self.kw = name, x, kw
        self.method = dc.METHODS[name] if composed is None else COMPOSED[name]
        self.args = {k: to_device(torch, v) if isinstance(v, np.ndarray) else copy.deepcopy(v)
                     for k, v in (kw if composed is None else composed).items()}
        if composed is None and name in dc.HAS_FIELD:
            self.args["field"] = field
        self.held = {}
        for arg, shape, dtype in dc.outputs(name, x.shape[0], kw):
            raw = torch.full((int(np.prod(shape)) * np.dtype(dtype).itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
            self.held[arg] = (raw, shape, dtype)
            self.args[arg] = raw.view(getattr(torch, dtype)).view(shape)
        self.returned = None

    def launch(self, ch):
        """The call, nothing waited for; the arguments are dropped with it: what they held is the kernel's or nobody's."""
        self.returned = getattr(ch, self.method)(self.x, **self.args)
        del self.args
        return self

    def result(self):
        """The host copies of what the call wrote, in the form of drawn_cases.mirror()."""
        arrays = {arg: raw.cpu().numpy().view(dtype).reshape(shape) for arg, (raw, shape, dtype) in self.held.items()}
        back = self.returned if isinstance(self.returned, tuple) else ()
        return dc.result(self.name, arrays, tuple(None if t is None else t.contiguous().cpu().numpy() for t in back), self.kw)


def synth(B, seed):
    """A tone per frame, 0.01 .. 0.45 of the sample rate, plus noise: float32 [B, N]."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    fb = rng.uniform(0.01, 0.45, size=B)
    return (0.8 * np.sin(2 * np.pi * fb[:, None] * n[None, :]) + 0.05 * rng.standard_normal((B, N))).astype(np.float32)


def table_window():
    """ones with a 1e-5 ripple at 3 cycles per frame: not a0 - a1 cos(2 pi n / (N-1)) (fit bound 1.5e-7), so the float
    kernels read the window table (WINGEN off).  Smooth by design: a sample read from the wrong place moves it by less
    than the gates notice; position errors are the business of window_cases.coded (tests/test_gpu_f32_window.py)."""
    n = np.arange(N)
    return (1.0 + 1e-5 * np.cos(2 * np.pi * 3 * n / N)).astype(np.float32)


def check_overlap_profiling_and_graph_capture(torch, ch, call, ref):
    """`call(out)` makes one process call into `out`; `ref` is the result of the plain stream-ordered call (after
    reserve).  Overlap depth 2 with flush, one device time per timed call, and capture into a graph: all outputs equal
    `ref`."""
    # overlap depth 2
    ch.set_overlap(2)
    outs = [torch.zeros_like(ref) for _ in range(3)]
    for o in outs:
        call(o)
    ch.flush()
    torch.cuda.synchronize()
    ch.set_overlap(1)
    for o in outs:
        assert torch.equal(o, ref)
    # launch timing: one time per call
    ch.set_profiling(4)
    out = torch.zeros_like(ref)
    for _ in range(3):
        call(out)
    ms = ch.profile_read(4)
    assert len(ms) == 3 and all(v > 0.0 for v in ms)
    ch.set_profiling(0)
    assert torch.equal(out, ref)
    # graph capture and replay
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        call(out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
