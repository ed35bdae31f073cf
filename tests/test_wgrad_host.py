"""CPU checks behind tests/test_wgrad_gpu.py: that wgrad_helpers.rounding_bound is neither vacuous nor too tight before
a GPU sees it, that the integer inputs really sum exactly in fp32, and how mlp._wgrad_launches cuts a job list into
launches.

The fp32 model sums as csrc/mlp.hip documents: a workgroup owns ceil(N / partials) rows rounded up to even and adds
their unfused products in one chain, the reduce kernel adds the partials in four groups and then ((g0+g1)+g2)+g3.  On
float_inputs it sits at 0.09 .. 0.15 of the bound for N <= 13, 0.013 at N = 257 and 0.002 at N = 4999.

A sum that lacks its last row must lie outside the bound.  With the integer inputs it does in every entry (the missing
product is at least 1); with the float inputs in every entry only while the sum has one or two terms: a product of two
clamped normals can be as small as 1e-6, below any bound proportional to the sum of 257 of them, so there the test asks
for nearly every entry and says how many."""
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import wgrad_helpers as H

SHAPES = [(32, 32), (31, 33), (1, 96), (33, 31), (64, 64), (63, 65)]     # (O, K), one per kernel variant


def _partials(N, O, K):
    from instag_amd import _lib
    p = H.partials(_lib.lib(), N, O, K)
    assert p == max(1, min(256, (N + 255) // 256))
    return p


def _model(dz, inp, partials):
    """fp32 dW summed in the kernel's partition of the rows (numpy, one rounding per operation)."""
    dz, inp = dz.numpy(), inp.numpy()
    N, O, K = dz.shape[0], dz.shape[1], inp.shape[1]
    per_block = (math.ceil(N / partials) + 1) & ~1
    parts = np.zeros((partials, O, K), dtype=np.float32)
    for b in range(partials):
        for r in range(b * per_block, min(N, (b + 1) * per_block)):
            prod = (dz[r][:, None] * inp[r][None, :]).astype(np.float32)
            parts[b] = (parts[b] + prod).astype(np.float32)
    per = (partials + 3) // 4
    groups = np.zeros((4, O, K), dtype=np.float32)
    for g in range(4):
        for p in range(g * per, min(partials, (g + 1) * per)):
            groups[g] = (groups[g] + parts[p]).astype(np.float32)
    return torch.from_numpy(((groups[0] + groups[1]) + groups[2]) + groups[3])


@pytest.mark.parametrize("N", [1, 2, 13, 257, 4999])
def test_fp32_model_of_the_partition_stays_within_the_bound(N):
    worst = 0.0
    for O, K in SHAPES:
        dz, inp = H.float_inputs(N, O, 1), H.float_inputs(N, K, 2)
        bound = H.rounding_bound(dz, inp, _partials(N, O, K))
        assert bound.shape == (O, K) and bool((bound > 0).all())
        ratio = float(((_model(dz, inp, _partials(N, O, K)).double() - H.reference(dz, inp)).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (N, O, K, ratio)
    print(f"N {N}: fp32 model at {worst:.4f} of the bound")


@pytest.mark.parametrize("N", [1, 2, 13, 257])
def test_a_dropped_row_exceeds_the_bound_in_every_entry(N):
    """The exact sum of all rows but the last is further from the reference than the bound allows, in every entry: with
    the integer inputs the missing product is at least 1 and the bound at most gamma_D * 9 N (0.02 at N = 257)."""
    for O, K in SHAPES:
        dz, inp = H.int_inputs(N, O, 1), H.int_inputs(N, K, 2)
        bound = H.rounding_bound(dz, inp, _partials(N, O, K))
        short = _model(dz[:N - 1], inp[:N - 1], 1) if N > 1 else torch.zeros(O, K)
        err = (short.double() - H.reference(dz, inp)).abs()
        assert bool((err > bound).all()), (N, O, K, float((err / bound).min()))


@pytest.mark.parametrize("N", [1, 2, 13, 257])
def test_a_dropped_row_of_float_inputs_exceeds_the_bound(N):
    """... and with the float inputs in every entry at N <= 2 (one or two terms against gamma_D < 1e-6) and in nearly
    every entry above: an entry escapes only where the missing product |x y| is below gamma_D * sum |x y|, about
    8.3e-6 * 257 * 0.64 = 1.4e-3 at N = 257, and P(|x y| < t) ~ (2 / pi) t (1 + ln(1 / t)) = 0.7 % of the entries for
    two normals; 2 % is allowed."""
    for O, K in SHAPES:
        dz, inp = H.float_inputs(N, O, 1), H.float_inputs(N, K, 2)
        bound = H.rounding_bound(dz, inp, _partials(N, O, K))
        short = _model(dz[:N - 1], inp[:N - 1], 1) if N > 1 else torch.zeros(O, K)
        over = ((short.double() - H.reference(dz, inp)).abs() > bound).double().mean()
        print(f"N {N} O {O} K {K}: {float(over):.4f} of the entries over the bound")
        assert float(over) == 1.0 if N <= 2 else float(over) >= 0.98, (N, O, K, float(over))


@pytest.mark.parametrize("N", [1, 13, 257, 65537])
def test_integer_inputs_sum_exactly_in_fp32(N):
    dz, inp = H.int_inputs(N, 64, 1), H.int_inputs(N, 96, 2)
    for t in (dz, inp):
        assert t.dtype == torch.float32 and bool((t == t.round()).all()) and bool((t != 0).all())
        assert float(t.abs().max()) <= 3 and bool((t < 0).any()) and bool((t > 0).any())
    ref = H.reference(dz, inp)
    assert torch.equal((dz.t() @ inp).double(), ref)
    assert float(ref.abs().max()) < 2 ** 24


def test_float_inputs_are_clamped_and_seeded():
    a, b = H.float_inputs(4999, 96, 5), H.float_inputs(4999, 96, 5)
    assert torch.equal(a, b) and not torch.equal(a, H.float_inputs(4999, 96, 6))
    assert float(a.abs().min()) >= 1e-3 and float(a.abs().max()) <= 8 and bool((a < 0).any()) and bool((a > 0).any())
    assert float(a.abs().min()) ** 3 > 1.2e-38          # a product of three is still normal in fp32


def test_virtual_rows_and_guarded():
    inp, aud, eye = H.int_inputs(5, 3, 1), H.int_inputs(5, 2, 2), H.int_inputs(5, 4, 3)
    enc_a, enc_e = H.int_inputs(2, None, 4), H.int_inputs(4, None, 5)
    rows = H.virtual_rows(inp, aud, eye, enc_a, enc_e)
    assert rows.shape == (5, 9) and rows.dtype == torch.float32
    assert torch.equal(rows[:, :3], inp) and torch.equal(rows[:, 3:5], aud * enc_a)
    assert torch.equal(rows[:, 5:], eye.clamp(min=0) * enc_e) and bool((eye < 0).any())
    g = H.guarded(inp, rows=2)
    assert torch.equal(g, inp) and g.is_contiguous()
    whole = g.untyped_storage()
    assert whole.nbytes() == 4 * 3 * 9 and g.storage_offset() == 6
    flat = torch.empty(0).set_(whole)
    assert bool(flat[:6].isnan().all()) and bool(flat[21:].isnan().all())


def _stand_in(N, virt):
    return (SimpleNamespace(shape=(N, 8)), SimpleNamespace(shape=(N, 8)), ("virt",) if virt else None)


@pytest.mark.parametrize("n_jobs", list(range(0, 41)))
def test_wgrad_launches_partition_any_job_list(n_jobs):
    from instag_amd.mlp import MAX_WGRAD_JOBS, _wgrad_launches
    assert MAX_WGRAD_JOBS == 16
    for trial in range(6):
        rng = random.Random(100 * n_jobs + trial)
        # one N only, two, or three; virtual jobs rare, frequent, or every job
        sizes = [257, 13, 65537][:1 + trial % 3]
        p_virt = (0.0, 0.1, 0.5, 1.0, 0.1, 0.5)[trial]
        jobs = [_stand_in(rng.choice(sizes), rng.random() < p_virt) for _ in range(n_jobs)]
        chunks = [list(c) for c in _wgrad_launches(jobs)]
        assert sorted(i for c in chunks for i in c) == list(range(n_jobs))
        assert (len(chunks) == 0) == (n_jobs == 0)
        for c in chunks:
            assert 1 <= len(c) <= MAX_WGRAD_JOBS
            assert len({jobs[i][0].shape[0] for i in c}) == 1
            assert sum(jobs[i][2] is not None for i in c) <= 1
        for N in sizes:
            order = [i for c in chunks for i in c if jobs[i][0].shape[0] == N]
            assert order == sorted(order)


def test_wgrad_launches_splits_two_virtual_jobs_of_one_size_and_seventeen_jobs():
    from instag_amd.mlp import _wgrad_launches
    jobs = [_stand_in(257, False), _stand_in(257, True), _stand_in(257, True), _stand_in(257, False)]
    assert [list(c) for c in _wgrad_launches(jobs)] == [[0, 1], [2, 3]]
    jobs = [_stand_in(13, False) for _ in range(17)]
    assert [list(c) for c in _wgrad_launches(jobs)] == [list(range(16)), [16]]
