"""CPU tests of tests/mlp_reference.py, the masked float64 reference of the classifier's training kernel:
it is the network of oracle/fdr_oracle.py, its generator is a sound restatement of mlp::uniform01, and the
data seeds of tests/mlp_exact_cases.py meet the ReLU knife-edge condition."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import mlp_exact_cases as E
import mlp_reference as R
from oracle import fdr_oracle
from test_fdr import CASES as FDR_CASES
from test_fdr import _random_problem


def test_random_problem_is_test_fdrs_generator():
    a = _random_problem(12, [100, 50, 20, 5])
    b = R.random_problem(12, 12, [100, 50, 20, 5])
    assert a[3] == b[3]
    for u, v in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(a[0].permutation(50), b[0].permutation(50))


@pytest.mark.parametrize("batch_size,d,layers", FDR_CASES)
def test_masked_fit_fp32_without_dropout_is_the_torch_oracle(batch_size, d, layers):
    """masked_fit(float32, dropout = 0) vs fdr_oracle.mlp_fit, two Adam steps with lr = 1, eps = 1 (the setting of
    test_hip_forward_backward_match_torch_fp32, where the parameter change is a smooth image of the gradient).
    The two differ by construction: torch's BatchNorm1d folds the normalisation into x * alpha + beta and sums the
    batch statistics in its own order, the functional form subtracts the mean first.  Measured on the four cases:
    parameter change 1.5e-8 ... 9.6e-7 (the largest change is 0.07 ... 0.20), loss 0 ... 1.9e-7 relative, running
    mean 1.0e-7 ... 3.4e-7 and running variance 1.0e-7 ... 2.8e-7 relative to max(|value|, 1).  Asserted with a 4x
    margin over the largest measured value of each."""
    rng, x, y, dims, params, rm, rv = _random_problem(d, layers)
    train_rows = rng.permutation(len(x))[: len(x) - 100]
    schedule = np.array([batch_size, 0], dtype=np.int64)
    adam = dict(betas=(0.9, 0.999), eps=1.0)
    ref = fdr_oracle.mlp_fit(dims, params, rm, rv, x, y, train_rows, schedule, batch_size, 1.0, 1e-5, **adam)
    got = R.masked_fit(torch.float32, dims, params, rm, rv, x, y, train_rows, schedule, batch_size, 1.0, 1e-5, 0.0, **adam)
    assert got.params.dtype == np.float32
    d_par = np.abs((got.params - params) - (ref[0] - params)).max()
    d_loss = np.abs(got.losses / ref[3].astype(np.float64) - 1).max()
    d_rm = (np.abs(got.rm - ref[1]) / np.maximum(np.abs(ref[1]), 1)).max()
    d_rv = (np.abs(got.rv - ref[2]) / np.maximum(np.abs(ref[2]), 1)).max()
    print(f"[masked_fit vs oracle] B={batch_size} d={d}: dparam {d_par:.2e} (largest change "
          f"{np.abs(ref[0] - params).max():.3f}), loss rel {d_loss:.2e}, rm {d_rm:.2e}, rv {d_rv:.2e}")
    assert np.abs(ref[0] - params).max() > 1e-4
    assert d_par < 4 * 9.6e-7
    assert d_loss < 4 * 1.9e-7
    assert d_rm < 4 * 3.4e-7
    assert d_rv < 4 * 2.8e-7


def test_masked_fit_continues_a_fit_from_its_moments():
    """first_step = k with the moments of the first k steps == all steps in one call (float64: to rounding)."""
    name = "tile-of-5-rows"
    c = E.BY_NAME[name]
    sched = np.array([c.batch_size, 0, 2 * c.batch_size, 0], dtype=np.int64)
    whole = E.fit_reference(name, torch.float64, sched)
    head = E.fit_reference(name, torch.float64, sched[:2])
    p = E.problem(name)
    tail = R.masked_fit(torch.float64, p.dims, head.params, head.rm, head.rv, p.x, p.y, p.train_rows, sched[2:],
                        c.batch_size, E.LR, E.WD, c.dropout, E.MASK_SEED, first_step=2, moments=head.moments, **E.ADAM)
    np.testing.assert_allclose(tail.params, whole.params, rtol=0, atol=1e-12)
    np.testing.assert_allclose(tail.losses, whole.losses[2:], rtol=1e-12)
    with pytest.raises(ValueError):
        E.fit_reference(name, torch.float64, sched[2:], first_step=2)


def _uniform01_python(seed, step, row, layer, j):
    """mlp::uniform01 in Python integers, the wrap-around written out."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (step + 1)) & m
    z ^= (row << 32) | (layer << 24) | j
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def test_uniform01_wraps_like_uint64():
    rng = np.random.default_rng(1)
    tuples = [(0, 0, 0, 0, 0), (2**64 - 1, 2**32 - 1, 2**31, 7, 1023), (E.MASK_SEED, 3, 255, 5, 271)]
    tuples += [(int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 10**6)), int(rng.integers(0, 4096)),
                int(rng.integers(0, 7)), int(rng.integers(0, 1024))) for _ in range(200)]
    for t in tuples:
        u = R.uniform01(*t)
        assert u.dtype == np.float32 and 0.0 <= float(u) < 1.0
        assert float(u) == _uniform01_python(*t), t
    # broadcasting over rows and units gives the scalar values
    grid = R.uniform01(E.MASK_SEED, 2, np.arange(5)[:, None], 1, np.arange(7)[None, :])
    assert grid.shape == (5, 7)
    assert float(grid[3, 6]) == _uniform01_python(E.MASK_SEED, 2, 3, 1, 6)


@pytest.mark.parametrize("p", [0.001, 0.3, 0.5])
def test_mask_statistics(p):
    """896 000 draws (14 steps x 5 layers x 128 rows x 100 units): the dropped fraction is p and the masks of
    neighbouring steps, layers and rows are independent (they agree on p^2 + (1 - p)^2 of the units), each within
    5 binomial standard deviations.  Measured: dropped 0.00095, 0.3002, 0.4998; agreement at p = 0.5 of 0.5010
    (steps), 0.4998 (layers), 0.4994 (rows)."""
    steps, layers, rows, units = 14, 5, 128, 100
    keep = np.stack([np.stack([R.keep_mask(E.MASK_SEED, s, l, rows, units, p) for l in range(layers)])
                     for s in range(steps)])
    n = keep.size
    assert n >= 500_000
    dropped = 1.0 - keep.mean()
    p32 = float(np.float32(p))
    assert abs(dropped - p32) < 5 * np.sqrt(p32 * (1 - p32) / n), dropped
    q = p32 * p32 + (1 - p32) * (1 - p32)
    for axis, a, b in (("steps", keep[1:], keep[:-1]), ("layers", keep[:, 1:], keep[:, :-1]),
                       ("rows", keep[:, :, 1:], keep[:, :, :-1]), ("units", keep[..., 1:], keep[..., :-1])):
        agree = float((a == b).mean())
        assert abs(agree - q) < 5 * np.sqrt(q * (1 - q) / a.size), (axis, agree, q)
    # another seed is another mask
    other = R.keep_mask(E.MASK_SEED + 1, 0, 0, rows, units, p)
    assert abs(float((other == keep[0, 0]).mean()) - q) < 5 * np.sqrt(q * (1 - q) / other.size)


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_case_seeds_meet_the_knife_edge_condition(name):
    """No hidden unit of a case is near enough to zero to change sign between float32 and float64 arithmetic
    (mlp_exact_cases.py), and the step moves something."""
    c, r = E.BY_NAME[name], E.references(name)
    for f32, f64 in ((r.one32, r.one64), (r.two32, r.two64)):
        zmin, err = R.knife_edge(f32, f64)
        print(f"[knife edge] {name}: smallest |z| {zmin:.2e}, float32 error {err:.2e}, noise "
              f"{E.noise(f32, f64, r.problem.params):.2e}, largest change {np.abs(f64.params - r.problem.params).max():.3f}")
        assert zmin > c.knife_margin * err
        assert np.abs(f64.params - r.problem.params).max() > 1e-4
