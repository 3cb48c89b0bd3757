"""Shared by the GPU test modules (a plain module, like structured_cases.py): the fixtures every one of them asks for,
imported by name into the module that uses them, and the helpers that were the same in two or more of them."""
import numpy as np
import pytest

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


def synth(B, seed):
    """A tone per frame, 0.01 .. 0.45 of the sample rate, plus noise: float32 [B, N]."""
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    fb = rng.uniform(0.01, 0.45, size=B)
    return (0.8 * np.sin(2 * np.pi * fb[:, None] * n[None, :]) + 0.05 * rng.standard_normal((B, N))).astype(np.float32)


def table_window():
    """ones with a 1e-5 ripple at 3 cycles per frame: not a0 - a1 cos(2 pi n / (N-1)) (fit bound 1.5e-7), so the float
    kernels read the window table (WINGEN off)."""
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
