"""CPU: the refusals of the reduction wrappers (reductions.py: fold_mag_f32, spectra_f32, find_peaks, peak_table_f32, order_stats,
noise_floor_f32, level_hist, persistence_f32, band_power, channel_power_f32, mask_test, mask_trigger_f32, harmonics,
harmonics_f32, find_signals, signals_f32, cfar, cfar_f32) as far as no device is needed, each pinned to its code and its full text, and the names the other tests and the
tools reach the tables and the libraries by.

Two objects stand in for a handle.  ``bare`` is ``object.__new__(SpectrumChain)``: nothing of it may be touched before the
scalar arguments and the input's type have passed.  ``host`` is the same with ``device`` set to the CPU, so that tensors in
host memory pass the input's check and the refusals behind it speak: the shapes, the limits, the batch, the outputs and the
workspace.  Every case ends in a refusal, so no library is loaded and nothing is launched.

The expected texts are those of the wrappers as they were before they shared one skeleton: the table was run against that
version and its output committed; the rows of the last four methods came with their libraries, and six rows of ``cfar``
with a bad ``field`` beside another fault when its field moved to the end of its rules, where every other method has it.  A row is (call, code, message); ``LIM`` is an object no check may look at, ``X``, ``REC`` and
``V`` good inputs ([2,16384], [2,16384,2] and [16384] float32) and ``BAD`` a tensor that is right for nothing.
"""
import numpy as np
import pytest

from conftest import N

CASES = [
    ('bare.fold_mag_f32(None, 3, 2)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.fold_mag_f32(None, 2, 3)', -1, 'bucket must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.fold_mag_f32(None, True, 2)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.fold_mag_f32(None, 2, 2.0)', -1, 'bucket must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.fold_mag_f32(None)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.fold_mag_f32(None, 2, 2)', -1, 'input must be a torch.float32 tensor'),
    ('host.fold_mag_f32(REC, 2, 2)', -2, 'input must be a contiguous [B, 16384] tensor'),
    ('host.fold_mag_f32(torch.zeros((3, N)), 2, 2)', -2, 'the batch (3 frames) must be a multiple of 2'),
    ('host.fold_mag_f32(X, 2, 2, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 8192, 2)'),
    ('host.fold_mag_f32(X, 2, 2, out=torch.zeros((1, N // 2, 2), dtype=torch.float64))', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 8192, 2)'),
    ('bare.spectra_f32(None, 3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.spectra_f32(None, 2, 3)', -1, 'bucket must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.spectra_f32(None, 1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.spectra_f32(None, 2)', -1, 'input must be a torch.float32 tensor'),
    ('host.spectra_f32(torch.zeros((2, N), dtype=torch.float64), 2)', -1, 'input must be a torch.float32 tensor'),
    ('host.spectra_f32(torch.zeros((3, N)), 2)', -2, 'the batch (3 frames) must be a multiple of 2'),
    ('host.spectra_f32(X, 2, 4, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 4096, 2)'),
    ('host.spectra_f32(torch.zeros((2, 24576), dtype=torch.uint8), 2, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 16384, 2)'),
    ('host.spectra_f32(torch.zeros((2, N), dtype=torch.int16), 2, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 16384, 2)'),
    ('host.spectra_f32(torch.zeros((2, N), dtype=torch.uint8), 2)', -2, 'input must be a contiguous [B, 24576] tensor'),
    ('bare.find_peaks(None, k=True)', -1, 'k must be an int'),
    ('bare.find_peaks(None, lo=0.0)', -1, 'lo must be an int'),
    ("bare.find_peaks(None, hi='5')", -1, 'hi must be an int'),
    ('bare.find_peaks(None, min_sep=2.0)', -1, 'min_sep must be an int'),
    ('bare.find_peaks(None, k=0)', -1, 'k must be 1..32'),
    ('bare.find_peaks(None, k=33)', -1, 'k must be 1..32'),
    ("bare.find_peaks(None, threshold='1')", -1, 'threshold must be a number'),
    ('bare.find_peaks(None, threshold=True)', -1, 'threshold must be a number'),
    ('bare.find_peaks(None, threshold=-1.0)', -1, 'threshold must be +0.0 .. +inf: no NaN, no sign bit'),
    ("bare.find_peaks(None, threshold=float('nan'))", -1, 'threshold must be +0.0 .. +inf: no NaN, no sign bit'),
    ('bare.find_peaks(None, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.find_peaks(None, hi=N + 1)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.find_peaks(None, min_sep=0)', -1, 'min_sep must be 1..16384'),
    ("bare.find_peaks(None, field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ('bare.find_peaks(None, field=0)', -1, "field must be None, 'peak' or 'power'"),
    ("bare.find_peaks(None, k=0, field='mag')", -1, 'k must be 1..32'),
    ('bare.find_peaks(None)', -1, 'input must be a torch.float32 tensor'),
    ("bare.find_peaks(None, field='peak')", -1, 'input must be a torch.float32 tensor'),
    ("host.find_peaks(X, field='power')", -2, 'input must be a contiguous [B, 16384, 2] tensor'),
    ('host.find_peaks(REC)', -2, 'input must be a contiguous [B, 16384] tensor'),
    ('host.find_peaks(X, k=4, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 4, 2)'),
    ("host.find_peaks(REC, field='peak', out=torch.zeros((2, 8, 2)))", -2, 'out must be a contiguous torch.int32 tensor of shape (2, 8, 2)'),
    ('bare.peak_table_f32(None, k=0, group=3)', -1, 'k must be 1..32'),
    ('bare.peak_table_f32(None, threshold=-1.0)', -1, 'threshold must be +0.0 .. +inf: no NaN, no sign bit'),
    ('bare.peak_table_f32(None, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.peak_table_f32(None, min_sep=True)', -1, 'min_sep must be an int'),
    ('bare.peak_table_f32(None, group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.peak_table_f32(None, group=1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.peak_table_f32(None, group=True)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.peak_table_f32(None, group=256)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.peak_table_f32(None, group=4)', -1, 'input must be a torch.float32 tensor'),
    ('bare.peak_table_f32(None)', -1, 'input must be a torch.float32 tensor'),
    ('host.peak_table_f32(X, group=4)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.peak_table_f32(X, group=2, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (1, 8, 2)'),
    ('host.peak_table_f32(X, k=3, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 3, 2)'),
    ('bare.order_stats(None, [0], lo=0.0)', -1, 'lo must be an int'),
    ('bare.order_stats(None, [0], hi=True)', -1, 'hi must be an int'),
    ('bare.order_stats(None, [0], lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ("bare.order_stats(None, '12')", -1, 'ranks must be a sequence of 1..8 ints'),
    ('bare.order_stats(None, 5)', -1, 'ranks must be a sequence of 1..8 ints'),
    ('bare.order_stats(None, [])', -1, 'ranks must be a sequence of 1..8 ints'),
    ('bare.order_stats(None, list(range(9)))', -1, 'ranks must be a sequence of 1..8 ints'),
    ('bare.order_stats(None, [1.0])', -1, 'a rank must be an int in 0..16383'),
    ('bare.order_stats(None, [N])', -1, 'a rank must be an int in 0..16383'),
    ('bare.order_stats(None, [10], lo=10, hi=20)', -1, 'a rank must be an int in 0..9'),
    ("bare.order_stats(None, [0], field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ("bare.order_stats(None, [N], field='mag')", -1, 'a rank must be an int in 0..16383'),
    ('bare.order_stats(None, [0, N - 1])', -1, 'input must be a torch.float32 tensor'),
    ("host.order_stats(X, [0], field='peak')", -2, 'input must be a contiguous [B, 16384, 2] tensor'),
    ('host.order_stats(X, [0, 5, 7], out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (2, 3)'),
    ("host.order_stats(REC, [0], field='power', out=torch.zeros((2, 1), dtype=torch.int32))", -2, 'out must be a contiguous torch.float32 tensor of shape (2, 1)'),
    ('bare.noise_floor_f32(None, lo=0.0)', -1, 'lo must be an int'),
    ('bare.noise_floor_f32(None, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.noise_floor_f32(None, q=[])', -1, 'q must be a number or a sequence of 1..8 numbers'),
    ('bare.noise_floor_f32(None, q=[0.5] * 9)', -1, 'q must be a number or a sequence of 1..8 numbers'),
    ('bare.noise_floor_f32(None, q=1.5)', -1, 'q must be a number in 0..1'),
    ('bare.noise_floor_f32(None, q=True)', -1, 'q must be a number in 0..1'),
    ("bare.noise_floor_f32(None, q='0.5')", -1, 'q must be a number in 0..1'),
    ('bare.noise_floor_f32(None, q=1.5, group=3)', -1, 'q must be a number in 0..1'),
    ('bare.noise_floor_f32(None, group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.noise_floor_f32(None, group=1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.noise_floor_f32(None, group=2.0)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.noise_floor_f32(None, group=8)', -1, 'input must be a torch.float32 tensor'),
    ('bare.noise_floor_f32(None)', -1, 'input must be a torch.float32 tensor'),
    ('host.noise_floor_f32(X, group=4)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.noise_floor_f32(X, q=(0.1, 0.9), group=2, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 2)'),
    ('host.noise_floor_f32(X, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (2, 1)'),
    ('bare.level_hist(None, [1.0], bucket=2.0)', -1, 'bucket must be an int'),
    ('bare.level_hist(None, [1.0], lo=True)', -1, 'lo must be an int'),
    ("bare.level_hist(None, [1.0], hi='8')", -1, 'hi must be an int'),
    ('bare.level_hist(None, [1.0], group=2.0)', -1, 'group must be an int'),
    ('bare.level_hist(None, [1.0], group=0)', -1, 'group must be 1..16777216'),
    ('bare.level_hist(None, [1.0], group=2 ** 24 + 1)', -1, 'group must be 1..16777216'),
    ('bare.level_hist(None, [1.0], bucket=3)', -1, 'bucket must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.level_hist(None, [])', -1, 'edges must be a sequence of 1..63 numbers'),
    ('bare.level_hist(None, [1.0] * 64)', -1, 'edges must be a sequence of 1..63 numbers'),
    ("bare.level_hist(None, ['1'])", -1, 'an edge must be a number'),
    ('bare.level_hist(None, [-1.0])', -1, 'an edge must be +0.0 .. +inf: no NaN, no sign bit'),
    ('bare.level_hist(None, [2.0, 1.0])', -1, 'the edges must not decrease'),
    ('bare.level_hist(None, [1.0], lo=8, hi=8)', -1, 'the range must be 0 <= lo < hi <= 16384, both multiples of the bucket'),
    ('bare.level_hist(None, [1.0], bucket=16, lo=8)', -1, 'the range must be 0 <= lo < hi <= 16384, both multiples of the bucket'),
    ('bare.level_hist(None, [], bucket=3)', -1, 'bucket must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.level_hist(None, [1.0, 2.0])', -1, 'input must be a torch.float32 tensor'),
    ('host.level_hist(REC, [1.0])', -2, 'input must be a contiguous [B, 16384] tensor'),
    ('host.level_hist(X, [1.0], group=3)', -2, 'the rows (2) must be a multiple of 3'),
    ('host.level_hist(X, [1.0, 2.0], bucket=16, out=BAD)', -2, 'out must be a contiguous torch.uint32 tensor of shape (1, 1024, 3)'),
    ('host.level_hist(X, [1.0], group=1, lo=16, hi=64, out=BAD)', -2, 'out must be a contiguous torch.uint32 tensor of shape (2, 48, 2)'),
    ('bare.persistence_f32(None, [1.0], bucket=2.0)', -1, 'bucket must be an int'),
    ('bare.persistence_f32(None, [1.0], group=0)', -1, 'group must be 1..16777216'),
    ('bare.persistence_f32(None, [1.0], group=True)', -1, 'group must be an int'),
    ('bare.persistence_f32(None, [1.0], bucket=3)', -1, 'bucket must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.persistence_f32(None, [2.0, 1.0])', -1, 'the edges must not decrease'),
    ('bare.persistence_f32(None, [1.0], lo=8)', -1, 'the range must be 0 <= lo < hi <= 16384, both multiples of the bucket'),
    ('bare.persistence_f32(None, [1.0], group=3)', -1, 'input must be a torch.float32 tensor'),
    ('bare.persistence_f32(None, [1.0])', -1, 'input must be a torch.float32 tensor'),
    ('host.persistence_f32(X, [1.0], group=3)', -2, 'the rows (2) must be a multiple of 3'),
    ('host.persistence_f32(X, [1.0], group=2, out=BAD)', -2, 'out must be a contiguous torch.uint32 tensor of shape (1, 1024, 2)'),
    ('host.persistence_f32(X, [1.0, 2.0], out=BAD)', -2, 'out must be a contiguous torch.uint32 tensor of shape (1, 1024, 3)'),
    ('bare.band_power(None, [])', -1, 'bands must be a sequence of 1..16 (lo, hi) pairs'),
    ('bare.band_power(None, [(0, 1)] * 17)', -1, 'bands must be a sequence of 1..16 (lo, hi) pairs'),
    ('bare.band_power(None, [5])', -1, 'a band must be a (lo, hi) pair'),
    ('bare.band_power(None, [(0.0, 5)])', -1, 'lo and hi of a band must be ints'),
    ('bare.band_power(None, [(5, 5)])', -1, 'a band must be 0 <= lo < hi <= 16384'),
    ('bare.band_power(None, [(0, 5)], fracs=0.5)', -1, 'fracs must be a sequence of 0..4 numbers'),
    ('bare.band_power(None, [(0, 5)], fracs=(0.5,) * 5)', -1, 'fracs must be a sequence of 0..4 numbers'),
    ('bare.band_power(None, [(0, 5)], fracs=(1.0,))', -1, 'a fraction must be a number in 0 .. 1 - 2^-32'),
    ("bare.band_power(None, [(0, 5)], field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ("bare.band_power(None, [(5, 5)], field='mag')", -1, 'a band must be 0 <= lo < hi <= 16384'),
    ('bare.band_power(None, [(0, 5)])', -1, 'input must be a torch.float32 tensor'),
    ("host.band_power(X, [(0, 5)], field='power')", -2, 'input must be a contiguous [B, 16384, 2] tensor'),
    ('host.band_power(X, [(0, 5), (7, 9)], power=BAD)', -2, 'power must be a contiguous torch.float64 tensor of shape (2, 2)'),
    ('host.band_power(X, [(0, 5), (7, 9)], (0.5,), power=BAD, cross=BAD)', -2, 'power must be a contiguous torch.float64 tensor of shape (2, 2)'),
    ('host.band_power(X, [(0, 5), (7, 9)], (0.5,), power=torch.zeros((2, 2), dtype=torch.float64), cross=BAD)', -2, 'cross must be a contiguous torch.int32 tensor of shape (2, 2, 1)'),
    ('bare.channel_power_f32(None, [])', -1, 'bands must be a sequence of 1..16 (lo, hi) pairs'),
    ('bare.channel_power_f32(None, [(5, 5)], group=3)', -1, 'a band must be 0 <= lo < hi <= 16384'),
    ('bare.channel_power_f32(None, [(0, 5)], fracs=(1.0,))', -1, 'a fraction must be a number in 0 .. 1 - 2^-32'),
    ('bare.channel_power_f32(None, [(0, 5)], group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.channel_power_f32(None, [(0, 5)], group=1)', -1, 'group = bucket = 1 folds nothing'),
    ("bare.channel_power_f32(None, [(0, 5)], group='4')", -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.channel_power_f32(None, [(0, 5)], group=4)', -1, 'input must be a torch.float32 tensor'),
    ('bare.channel_power_f32(None, [(0, 5)])', -1, 'input must be a torch.float32 tensor'),
    ('host.channel_power_f32(X, [(0, 5)], group=4)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.channel_power_f32(X, [(0, 5)], group=2, power=BAD)', -2, 'power must be a contiguous torch.float64 tensor of shape (1, 1)'),
    ('host.channel_power_f32(X, [(0, 5)], (0.5, 0.1), power=torch.zeros((2, 1), dtype=torch.float64), cross=BAD)', -2, 'cross must be a contiguous torch.int32 tensor of shape (2, 1, 2)'),
    ('bare.mask_test(None, LIM, lo=0.0)', -1, 'lo must be an int'),
    ('bare.mask_test(None, LIM, hi=True)', -1, 'hi must be an int'),
    ('bare.mask_test(None, LIM, lo=6, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ("bare.mask_test(None, LIM, field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ('bare.mask_test(None, None)', -1, 'upper and lower are both None: no limit at all'),
    ('bare.mask_test(None, None, lo=6, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.mask_test(None, LIM)', -1, 'input must be a torch.float32 tensor'),
    ("bare.mask_test(None, None, LIM, field='peak')", -1, 'input must be a torch.float32 tensor'),
    ('host.mask_test(REC, LIM)', -2, 'input must be a contiguous [B, 16384] tensor'),
    ('host.mask_test(X, LIM)', -2, 'upper must be None or a contiguous torch.float32 tensor of shape (16384,)'),
    ('host.mask_test(X, V, LIM)', -2, 'lower must be None or a contiguous torch.float32 tensor of shape (16384,)'),
    ('host.mask_test(X, V, torch.zeros(N, dtype=torch.float64))', -2, 'lower must be None or a contiguous torch.float32 tensor of shape (16384,)'),
    ('host.mask_test(X, V, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 10)'),
    ('host.mask_test(X, V, out=BAD, summary=True)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 10)'),
    ('host.mask_test(X, V, V, out=torch.zeros((2, 10), dtype=torch.int32), summary=BAD)', -2, 'summary must be a contiguous torch.int32 tensor of shape (4,)'),
    ('bare.mask_trigger_f32(None, LIM, lo=0.0)', -1, 'lo must be an int'),
    ('bare.mask_trigger_f32(None, LIM, lo=6, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.mask_trigger_f32(None, None)', -1, 'upper and lower are both None: no limit at all'),
    ('bare.mask_trigger_f32(None, None, group=3)', -1, 'upper and lower are both None: no limit at all'),
    ('bare.mask_trigger_f32(None, LIM, group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.mask_trigger_f32(None, LIM, group=1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.mask_trigger_f32(None, LIM, group=0)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.mask_trigger_f32(None, LIM, group=4)', -1, 'input must be a torch.float32 tensor'),
    ('bare.mask_trigger_f32(None, LIM, summary=True)', -1, 'input must be a torch.float32 tensor'),
    ('bare.mask_trigger_f32(None, LIM)', -1, 'input must be a torch.float32 tensor'),
    ('host.mask_trigger_f32(X, LIM, summary=True, group=4)', -2, 'upper must be None or a contiguous torch.float32 tensor of shape (16384,)'),
    ('host.mask_trigger_f32(X, V, LIM, summary=False)', -2, 'lower must be None or a contiguous torch.float32 tensor of shape (16384,)'),
    ('host.mask_trigger_f32(X, V, summary=True, group=4)', -2, 'summary must be None or a contiguous torch.int32 tensor of shape (4,)'),
    ('host.mask_trigger_f32(X, V, summary=False, out=BAD)', -2, 'summary must be None or a contiguous torch.int32 tensor of shape (4,)'),
    ('host.mask_trigger_f32(X, V, group=4, out=BAD)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.mask_trigger_f32(X, V, group=2, out=BAD, summary=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (1, 10)'),
    ('host.mask_trigger_f32(X, V, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 10)'),
    ('host.mask_trigger_f32(X, V, out=torch.zeros((2, 10), dtype=torch.int32), summary=BAD)', -2, 'summary must be a contiguous torch.int32 tensor of shape (4,)'),
    ('bare.harmonics(None, order=2.0)', -1, 'order must be an int'),
    ('bare.harmonics(None, span=True)', -1, 'span must be an int'),
    ("bare.harmonics(None, lo='1')", -1, 'lo must be an int'),
    ('bare.harmonics(None, fund=1.0)', -1, 'fund must be an int'),
    ('bare.harmonics(None, dc=False)', -1, 'dc must be an int'),
    ('bare.harmonics(None, top=8193.0)', -1, 'top must be an int'),
    ('bare.harmonics(None, span=65)', -1, 'span must be 0..64'),
    ('bare.harmonics(None, order=0)', -1, 'order must be 1..10'),
    ('bare.harmonics(None, order=11)', -1, 'order must be 1..10'),
    ('bare.harmonics(None, dc=9000)', -1, 'the analysed bins must be 0 <= dc < top <= 8193'),
    ('bare.harmonics(None, top=8194)', -1, 'the analysed bins must be 0 <= dc < top <= 8193'),
    ('bare.harmonics(None, lo=2)', -1, 'the search range must be dc <= lo < hi <= top'),
    ('bare.harmonics(None, lo=50, hi=50)', -1, 'the search range must be dc <= lo < hi <= top'),
    ('bare.harmonics(None, fund=2)', -1, 'fund must be None, -1 or a bin in [dc, top)'),
    ("bare.harmonics(None, field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ("bare.harmonics(None, order=0, field='mag')", -1, 'order must be 1..10'),
    ('bare.harmonics(None)', -1, 'input must be a torch.float32 tensor'),
    ("bare.harmonics(None, fund=-1, field='power')", -1, 'input must be a torch.float32 tensor'),
    ("host.harmonics(X, field='peak')", -2, 'input must be a contiguous [B, 16384, 2] tensor'),
    ('host.harmonics(X, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 42)'),
    ("host.harmonics(REC, field='power', out=torch.zeros((2, 42)))", -2, 'out must be a contiguous torch.int32 tensor of shape (2, 42)'),
    ('bare.harmonics_f32(None, order=0)', -1, 'order must be 1..10'),
    ('bare.harmonics_f32(None, span=65, group=3)', -1, 'span must be 0..64'),
    ('bare.harmonics_f32(None, fund=2)', -1, 'fund must be None, -1 or a bin in [dc, top)'),
    ('bare.harmonics_f32(None, group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.harmonics_f32(None, group=1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.harmonics_f32(None, group=2.0)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.harmonics_f32(None, group=128)', -1, 'input must be a torch.float32 tensor'),
    ('bare.harmonics_f32(None)', -1, 'input must be a torch.float32 tensor'),
    ('host.harmonics_f32(X, group=4)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.harmonics_f32(X, group=2, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (1, 42)'),
    ('host.harmonics_f32(X, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 42)'),
    ('host.spectra_f32(X, 2, work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.peak_table_f32(X, work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.peak_table_f32(X, group=2, work=torch.zeros((1, N)))', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.noise_floor_f32(X, work=torch.zeros((2, N), dtype=torch.float64))', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.persistence_f32(X, [1.0], work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.channel_power_f32(X, [(0, 5)], (0.5,), work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.mask_trigger_f32(X, V, work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.harmonics_f32(X, group=2, work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('bare.find_signals(None, k=True)', -1, 'k must be an int'),
    ('bare.find_signals(None, lo=0.0)', -1, 'lo must be an int'),
    ("bare.find_signals(None, hi='5')", -1, 'hi must be an int'),
    ('bare.find_signals(None, gap=2.0)', -1, 'gap must be an int'),
    ('bare.find_signals(None, min_width=False)', -1, 'min_width must be an int'),
    ('bare.find_signals(None, k=0)', -1, 'k must be 1..32'),
    ('bare.find_signals(None, k=33)', -1, 'k must be 1..32'),
    ('bare.find_signals(None, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.find_signals(None, hi=N + 1)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.find_signals(None, gap=-1)', -1, 'gap must be 0..16383'),
    ('bare.find_signals(None, gap=N)', -1, 'gap must be 0..16383'),
    ('bare.find_signals(None, min_width=0)', -1, 'min_width must be 1..16384'),
    ('bare.find_signals(None, min_width=N + 1)', -1, 'min_width must be 1..16384'),
    ("bare.find_signals(None, field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ('bare.find_signals(None, field=0)', -1, "field must be None, 'peak' or 'power'"),
    ("bare.find_signals(None, k=0, field='mag')", -1, 'k must be 1..32'),
    ("bare.find_signals(None, threshold='1')", -1, 'threshold must be a number'),
    ('bare.find_signals(None, threshold=True)', -1, 'threshold must be a number'),
    ('bare.find_signals(None, threshold=None)', -1, 'threshold must be a number'),
    ('bare.find_signals(None, threshold=-1.0)', -1, 'threshold must be +0.0 .. +inf: no NaN, no sign bit'),
    ("bare.find_signals(None, threshold=float('nan'))", -1, 'threshold must be +0.0 .. +inf: no NaN, no sign bit'),
    ('bare.find_signals(None, threshold=torch.zeros(2, dtype=torch.float64))', -1, 'a threshold per row must be a torch.float32 tensor'),
    ('bare.find_signals(None, threshold=torch.zeros(2, dtype=torch.int32))', -1, 'a threshold per row must be a torch.float32 tensor'),
    ('bare.find_signals(None)', -1, 'input must be a torch.float32 tensor'),
    ("bare.find_signals(None, threshold=torch.zeros(2), field='peak')", -1, 'input must be a torch.float32 tensor'),
    ("host.find_signals(X, field='power')", -2, 'input must be a contiguous [B, 16384, 2] tensor'),
    ('host.find_signals(REC)', -2, 'input must be a contiguous [B, 16384] tensor'),
    ('host.find_signals(X, threshold=torch.zeros(3))', -2, 'a threshold per row must be a contiguous torch.float32 tensor of shape (2,)'),
    ('host.find_signals(X, threshold=torch.zeros((2, 1)))', -2, 'a threshold per row must be a contiguous torch.float32 tensor of shape (2,)'),
    ('host.find_signals(X, threshold=torch.zeros(4)[::2])', -2, 'a threshold per row must be a contiguous torch.float32 tensor of shape (2,)'),
    ('host.find_signals(X, threshold=torch.zeros(3), out=BAD)', -2, 'a threshold per row must be a contiguous torch.float32 tensor of shape (2,)'),
    ('host.find_signals(X, k=4, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 4, 6)'),
    ("host.find_signals(REC, field='peak', out=torch.zeros((2, 16, 6)))", -2, 'out must be a contiguous torch.int32 tensor of shape (2, 16, 6)'),
    ('host.find_signals(X, k=4, out=BAD, stats=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 4, 6)'),
    ('host.find_signals(X, k=4, stats=BAD)', -2, 'stats must be a contiguous torch.int32 tensor of shape (2, 3)'),
    ('host.find_signals(X, k=4, out=torch.zeros((2, 4, 6), dtype=torch.int32), stats=torch.zeros((2, 3)))', -2, 'stats must be a contiguous torch.int32 tensor of shape (2, 3)'),
    ('bare.signals_f32(None)', -1, 'exactly one of threshold and factor must be given'),
    ('bare.signals_f32(None, threshold=1.0, factor=6.0)', -1, 'exactly one of threshold and factor must be given'),
    ('bare.signals_f32(None, threshold=torch.zeros(2), factor=6)', -1, 'exactly one of threshold and factor must be given'),
    ('bare.signals_f32(None, k=0)', -1, 'k must be 1..32'),
    ('bare.signals_f32(None, k=0, threshold=1.0, factor=6.0, group=3)', -1, 'k must be 1..32'),
    ('bare.signals_f32(None, factor=6.0, gap=N)', -1, 'gap must be 0..16383'),
    ('bare.signals_f32(None, threshold=1.0, min_width=2.0)', -1, 'min_width must be an int'),
    ('bare.signals_f32(None, threshold=1.0, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.signals_f32(None, threshold=-1.0)', -1, 'threshold must be +0.0 .. +inf: no NaN, no sign bit'),
    ("bare.signals_f32(None, threshold='1')", -1, 'threshold must be a number'),
    ('bare.signals_f32(None, threshold=torch.zeros(2, dtype=torch.float64))', -1, 'a threshold per row must be a torch.float32 tensor'),
    ('bare.signals_f32(None, factor=0.0)', -1, 'factor must be a finite number above 0 as a float32'),
    ('bare.signals_f32(None, factor=-6.0)', -1, 'factor must be a finite number above 0 as a float32'),
    ("bare.signals_f32(None, factor=float('inf'))", -1, 'factor must be a finite number above 0 as a float32'),
    ("bare.signals_f32(None, factor=float('nan'))", -1, 'factor must be a finite number above 0 as a float32'),
    ('bare.signals_f32(None, factor=1e-50)', -1, 'factor must be a finite number above 0 as a float32'),
    ('bare.signals_f32(None, factor=1e39)', -1, 'factor must be a finite number above 0 as a float32'),
    ('bare.signals_f32(None, factor=True)', -1, 'factor must be a finite number above 0 as a float32'),
    ("bare.signals_f32(None, factor='6')", -1, 'factor must be a finite number above 0 as a float32'),
    ('bare.signals_f32(None, factor=6.0, q=1.5)', -1, 'q must be a number in 0..1'),
    ('bare.signals_f32(None, factor=6.0, q=[0.5])', -1, 'q must be a number in 0..1'),
    ('bare.signals_f32(None, factor=6.0, q=True)', -1, 'q must be a number in 0..1'),
    ('bare.signals_f32(None, factor=6.0, q=1.5, group=3)', -1, 'q must be a number in 0..1'),
    ('bare.signals_f32(None, factor=6.0, group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.signals_f32(None, threshold=1.0, group=1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.signals_f32(None, threshold=1.0, group=2.0)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.signals_f32(None, factor=6.0, group=128)', -1, 'input must be a torch.float32 tensor'),
    ('bare.signals_f32(None, threshold=1.0)', -1, 'input must be a torch.float32 tensor'),
    ('host.signals_f32(X, factor=6.0, group=4)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.signals_f32(X, threshold=torch.zeros(2), group=2)', -2, 'a threshold per row must be a contiguous torch.float32 tensor of shape (1,)'),
    ('host.signals_f32(X, threshold=torch.zeros(3))', -2, 'a threshold per row must be a contiguous torch.float32 tensor of shape (2,)'),
    ('host.signals_f32(X, factor=6.0, group=2, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (1, 16, 6)'),
    ('host.signals_f32(X, threshold=1.0, k=3, out=BAD)', -2, 'out must be a contiguous torch.int32 tensor of shape (2, 3, 6)'),
    ('host.signals_f32(X, factor=6.0, stats=BAD)', -2, 'stats must be a contiguous torch.int32 tensor of shape (2, 3)'),
    ('host.signals_f32(X, factor=6.0, work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.signals_f32(X, threshold=1.0, group=2, work=torch.zeros((1, N)))', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('bare.cfar(None, train=True)', -1, 'train must be an int'),
    ('bare.cfar(None, train=16.0)', -1, 'train must be an int'),
    ('bare.cfar(None, guard=2.0)', -1, 'guard must be an int'),
    ('bare.cfar(None, guard=False)', -1, 'guard must be an int'),
    ('bare.cfar(None, lo=0.0)', -1, 'lo must be an int'),
    ("bare.cfar(None, hi='5')", -1, 'hi must be an int'),
    ('bare.cfar(None, train=3)', -1, 'train must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.cfar(None, train=0)', -1, 'train must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.cfar(None, train=128)', -1, 'train must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.cfar(None, guard=-1)', -1, 'guard must be 0..64'),
    ('bare.cfar(None, guard=65)', -1, 'guard must be 0..64'),
    ("bare.cfar(None, mode='os')", -1, "mode must be 'ca', 'go' or 'so'"),
    ('bare.cfar(None, mode=0)', -1, "mode must be 'ca', 'go' or 'so'"),
    ("bare.cfar(None, what='db')", -1, "what must be 'ratio' or 'floor'"),
    ('bare.cfar(None, what=1)', -1, "what must be 'ratio' or 'floor'"),
    ('bare.cfar(None, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.cfar(None, hi=N + 1)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.cfar(None, lo=10, hi=15)', -1, 'the range must hold 2 * guard + 2 bins or more'),
    ('bare.cfar(None, guard=64, lo=0, hi=129)', -1, 'the range must hold 2 * guard + 2 bins or more'),
    ("bare.cfar(None, field='mag')", -1, "field must be None, 'peak' or 'power'"),
    ('bare.cfar(None, field=0)', -1, "field must be None, 'peak' or 'power'"),
    ("bare.cfar(None, train=True, field='mag')", -1, 'train must be an int'),
    ("bare.cfar(None, train=3, field='mag')", -1, 'train must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.cfar(None, guard=65, field=0)', -1, 'guard must be 0..64'),
    ("bare.cfar(None, mode='os', field='mag')", -1, "mode must be 'ca', 'go' or 'so'"),
    ("bare.cfar(None, what='db', field='mag')", -1, "what must be 'ratio' or 'floor'"),
    ("bare.cfar(None, lo=5, hi=5, field='mag')", -1, 'the range must be 0 <= lo < hi <= 16384'),
    ("bare.cfar(None, lo=10, hi=15, field='mag')", -1, 'the range must hold 2 * guard + 2 bins or more'),
    ('bare.cfar(None)', -1, 'input must be a torch.float32 tensor'),
    ("bare.cfar(None, 64, 64, 'so', 'floor', 0, 130, 'power')", -1, 'input must be a torch.float32 tensor'),
    ("host.cfar(X, field='power')", -2, 'input must be a contiguous [B, 16384, 2] tensor'),
    ('host.cfar(REC)', -2, 'input must be a contiguous [B, 16384] tensor'),
    ('host.cfar(X, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (2, 16384)'),
    ('host.cfar(X, out=torch.zeros((2, N), dtype=torch.float64))', -2, 'out must be a contiguous torch.float32 tensor of shape (2, 16384)'),
    ("host.cfar(REC, field='peak', out=torch.zeros((2, N, 2)))", -2, 'out must be a contiguous torch.float32 tensor of shape (2, 16384)'),
    ('bare.cfar_f32(None, train=5)', -1, 'train must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.cfar_f32(None, train=5, group=3)', -1, 'train must be one of (1, 2, 4, 8, 16, 32, 64)'),
    ('bare.cfar_f32(None, guard=1.5)', -1, 'guard must be an int'),
    ('bare.cfar_f32(None, guard=100)', -1, 'guard must be 0..64'),
    ("bare.cfar_f32(None, mode='CA')", -1, "mode must be 'ca', 'go' or 'so'"),
    ("bare.cfar_f32(None, what='snr')", -1, "what must be 'ratio' or 'floor'"),
    ('bare.cfar_f32(None, lo=5, hi=5)', -1, 'the range must be 0 <= lo < hi <= 16384'),
    ('bare.cfar_f32(None, lo=0, hi=5)', -1, 'the range must hold 2 * guard + 2 bins or more'),
    ('bare.cfar_f32(None, group=3)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.cfar_f32(None, group=1)', -1, 'group = bucket = 1 folds nothing'),
    ('bare.cfar_f32(None, group=2.0)', -1, 'group must be one of (1, 2, 4, 8, 16, 32, 64, 128)'),
    ('bare.cfar_f32(None, group=128)', -1, 'input must be a torch.float32 tensor'),
    ('bare.cfar_f32(None)', -1, 'input must be a torch.float32 tensor'),
    ('host.cfar_f32(X, group=4)', -2, 'the batch (2 frames) must be a multiple of 4'),
    ('host.cfar_f32(X, group=2, out=torch.zeros((2, N)))', -2, 'out must be a contiguous torch.float32 tensor of shape (1, 16384)'),
    ('host.cfar_f32(X, out=BAD)', -2, 'out must be a contiguous torch.float32 tensor of shape (2, 16384)'),
    ('host.cfar_f32(X, work=BAD)', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
    ('host.cfar_f32(X, group=2, work=torch.zeros((1, N)))', -2, 'work must be a contiguous torch.float32 tensor of shape [2 or more, 16384]'),
]
METHODS = ("fold_mag_f32", "spectra_f32", "find_peaks", "peak_table_f32", "order_stats", "noise_floor_f32", "level_hist",
           "persistence_f32", "band_power", "channel_power_f32", "mask_test", "mask_trigger_f32", "harmonics", "harmonics_f32",
           "find_signals", "signals_f32", "cfar", "cfar_f32")
# the methods whose tables came with a floor of 8 distinct scalar refusals
MANY_TEXTS = ("find_signals", "signals_f32", "cfar", "cfar_f32")
COMPOSED = ("peak_table_f32", "noise_floor_f32", "persistence_f32", "channel_power_f32", "mask_trigger_f32", "harmonics_f32",
            "signals_f32", "cfar_f32")


def _namespace():
    import torch

    from fpga_real_time_fft_analyzer_amd.chain import SpectrumChain
    bare, host = object.__new__(SpectrumChain), object.__new__(SpectrumChain)
    host.device = torch.device("cpu")
    return dict(bare=bare, host=host, LIM=object(), np=np, N=N, torch=torch, X=torch.zeros((2, N)), REC=torch.zeros((2, N, 2)),
                V=torch.zeros(N), BAD=torch.zeros(3))


def test_every_refusal_keeps_its_code_and_its_text():
    from fpga_real_time_fft_analyzer_amd.abi import SpecanError
    ns = _namespace()
    assert len({call for call, _, _ in CASES}) == len(CASES)
    for call, code, message in CASES:
        with pytest.raises(SpecanError) as e:
            eval(call, ns)
        assert (e.value.code, str(e.value)) == (code, f"specan error {code}: {message}"), call


def _rows(method, obj=""):
    """call -> message of the rows of ``method``, those on ``obj`` ('bare' or 'host') where one is named."""
    return {call: message for call, _, message in CASES if f".{method}(" in call and call.startswith(obj)}


def test_the_table_covers_every_method():
    """Each of the eighteen methods has a scalar refusal, and with good arguments the refusal of its input; a bad argument wins
    over a bad input (every ``bare`` row passes None as the input); the composed ones have their ``group`` refusals."""
    groups = "group must be one of (1, 2, 4, 8, 16, 32, 64, 128)"
    for method in METHODS:
        texts = list(_rows(method, "bare").values())
        assert "input must be a torch.float32 tensor" in texts and len(set(texts)) >= (8 if method in MANY_TEXTS else 4), method
        assert any(" must be " in t and "tensor" not in t for t in texts), method
        assert any("shape" in message for message in _rows(method, "host").values()), method
    for method in COMPOSED:
        texts = _rows(method)
        if method == "persistence_f32":               # its group is the histogram's: any number of rows, and no fold
            assert texts["bare.persistence_f32(None, [1.0], group=0)"] == "group must be 1..16777216"
            assert texts["bare.persistence_f32(None, [1.0], group=3)"] == "input must be a torch.float32 tensor"
            assert texts["host.persistence_f32(X, [1.0], group=3)"] == "the rows (2) must be a multiple of 3"
            continue
        assert groups in texts.values() and "group = bucket = 1 folds nothing" in texts.values(), method
        assert "the batch (2 frames) must be a multiple of 4" in texts.values(), method
    texts = _rows("mask_trigger_f32")
    limits = "upper must be None or a contiguous torch.float32 tensor of shape (16384,)"
    summary = "summary must be None or a contiguous torch.int32 tensor of shape (4,)"
    assert texts["bare.mask_trigger_f32(None, LIM, summary=True)"] == "input must be a torch.float32 tensor"      # the input first,
    assert texts["host.mask_trigger_f32(X, LIM, summary=True, group=4)"] == limits                                 # then the limits,
    assert texts["host.mask_trigger_f32(X, V, summary=True, group=4)"] == summary                                  # a bool summary,
    assert texts["host.mask_trigger_f32(X, V, group=4, out=BAD)"] == "the batch (2 frames) must be a multiple of 4"  # the batch
    assert texts["host.mask_trigger_f32(X, V, out=torch.zeros((2, 10), dtype=torch.int32), summary=BAD)"].startswith("summary must be a")
    assert _rows("peak_table_f32")["bare.peak_table_f32(None, group=1)"] == "group = bucket = 1 folds nothing"


def test_the_names_the_tests_and_tools_use():
    import os

    from fpga_real_time_fft_analyzer_amd import abi, chain
    from reduction_libraries import LIBRARIES
    assert chain.reductions.FIELDS == {None: 0, "peak": 1, "power": 2} and chain._HARM_WORDS == 42
    for x in LIBRARIES:
        if x not in ("fold", "hist"):                 # these two take magnitudes only
            assert [getattr(abi, f"SA_{x.upper()}_IN_{k}") for k in ("MAG", "POINT_PEAK", "POINT_POWER")] == [0, 1, 2], x
        path, load = getattr(abi, f"{x.upper()}_LIB_PATH"), getattr(abi, f"{x}_lib")
        assert path == os.path.join(os.path.dirname(abi.LIB_PATH), f"libspecan_{x}.so"), x
        assert callable(load) and load.__name__ == f"{x}_lib" and f"libspecan_{x}.so" in load.__doc__ and f"specan_{x}.h" in load.__doc__
        assert f"sa_{x}_last_error" in getattr(abi, f"{x.upper()}_SIGNATURES"), x
    cls = chain.SpectrumChain
    for name in METHODS + ("_peaks_args", "_rank_args", "_quantile_ranks", "_hist_args", "_bands_args", "_mask_args", "_harm_args",
                           "_log2_fold"):
        assert callable(getattr(cls, name)), name
    assert cls._log2_fold(4, 2) == (2, 1) and cls._peaks_args(8, 0.0, 0, N, 1, "power") == 2
