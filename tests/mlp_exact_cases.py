"""The cases of tests/test_mlp_exact_gpu.py and their CPU references (tests/mlp_reference.py), computed once.

TEST INFRASTRUCTURE.  Every case is (batch_size, d, hidden layers, output_dim, dropout), chosen for the path
of alphadia_amd/csrc/adh_mlp.hip it reaches; the number in brackets is the count of 16-column blocks of the
widest hidden layer, which the 8 waves of a workgroup take in rounds of 8.

DATA_SEED is the seed of ``mlp_reference.random_problem`` for the case.  It is searched on the CPU, from the two
references alone, for the ReLU knife-edge condition: over both steps compared, the float64 run's smallest
|pre-activation| must exceed KNIFE_MARGIN times the largest float32 - float64 pre-activation difference, so
that no hidden unit can change sign between the device and the arbiter (one flipped unit moves a parameter by
~3e-5, six times the bound).  The margin is 64 wherever data can meet it.  The seven-Linear case compares
2 x 256 x 188 = 96 256 pre-activations whose float32 error is 1e-6 (a 70-term dot product): their smallest
|z| is ~5e-6 on average, 3000 seeds gave at most 20.6 times the error, and 64 would need a seed in ~1e8.  That
case asserts 16, the factor the parameter bound itself allows the device over the float32 noise.
tests/test_mlp_reference.py asserts the condition for every case without a GPU.
"""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import mlp_reference as R

Case = namedtuple("Case", "name batch_size d layers output_dim dropout data_seed knife_margin")

CASES = [
    Case("production-p0.5", 128, 12, [100, 50, 20, 5], 2, 0.5, 188, 64),          # [7] the production architecture
    Case("production-p0.001", 100, 46, [100, 50, 20, 5], 2, 0.001, 4602, 64),     # production rate; partial last tile
    Case("tile-of-5-rows", 37, 5, [8], 2, 0.5, 5, 64),                            # 37 = 2 * 16 + 5
    Case("seven-linears", 256, 70, [64, 64, 32, 16, 8, 4], 2, 0.3, 605, 16),      # input rows not in registers
    Case("9-blocks", 48, 12, [144, 8], 2, 0.5, 13, 64),                           # [9] a second round for wave 0
    Case("17-blocks-p0", 33, 20, [272], 2, 0.0, 20, 64),                          # [17] three rounds
    Case("17-blocks-p0.5", 33, 20, [272], 2, 0.5, 20, 64),
    Case("batch-of-2", 2, 3, [4], 2, 0.5, 3, 64),                                 # the smallest legal batch
    Case("no-hidden-layer", 64, 9, [], 2, 0.0, 9, 64),                            # n_linear = 1: backward for l = 0 only
    Case("3-classes", 80, 12, [24, 8], 3, 0.3, 12, 64),                           # targets of classes >= 2 are 0
    Case("8-classes", 80, 12, [24, 8], 8, 0.3, 13, 64),                           # the ABI's maximum
]
BY_NAME = {c.name: c for c in CASES}

MASK_SEED = 0x5EED1234ABCD  # wider than 32 bits: the hash takes the seed as uint64
LR, WD, ADAM = 1.0, 1e-5, dict(betas=(0.9, 0.999), eps=1.0)

Problem = namedtuple("Problem", "x y dims params rm rv train_rows schedule")
Refs = namedtuple("Refs", "problem one32 one64 two32 two64")


@functools.lru_cache(maxsize=None)
def problem(name: str) -> Problem:
    c = BY_NAME[name]
    rng, x, y, dims, params, rm, rv = R.random_problem(c.data_seed, c.d, c.layers, c.output_dim)
    train_rows = rng.permutation(len(x))[: len(x) - 100]
    for a in (x, y, params, rm, rv, train_rows):
        a.setflags(write=False)
    return Problem(x, y, dims, params, rm, rv, train_rows, np.array([c.batch_size, 0], dtype=np.int64))


def fit_reference(name: str, dtype, schedule, seed=MASK_SEED, lr=LR, **kw):
    c, p = BY_NAME[name], problem(name)
    return R.masked_fit(dtype, p.dims, p.params, p.rm, p.rv, p.x, p.y, p.train_rows, schedule, c.batch_size, lr, WD,
                        c.dropout, seed, **dict(ADAM, **kw))


@functools.lru_cache(maxsize=None)
def references(name: str) -> Refs:
    """One step and two steps from the case's state, in float32 and float64."""
    import torch

    p = problem(name)
    return Refs(p, fit_reference(name, torch.float32, p.schedule[:1]), fit_reference(name, torch.float64, p.schedule[:1]),
                fit_reference(name, torch.float32, p.schedule), fit_reference(name, torch.float64, p.schedule))


def noise(fit32, fit64, params) -> float:
    """max |delta param float32 - delta param float64|: what float32 arithmetic alone does to the comparison."""
    p0 = np.asarray(params, np.float64)
    return float(np.abs((fit32.params.astype(np.float64) - p0) - (fit64.params - p0)).max())
