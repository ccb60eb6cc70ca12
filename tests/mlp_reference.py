"""A CPU reference of the classifier's training step that applies the device's own dropout masks.

TEST INFRASTRUCTURE.  ``oracle/fdr_oracle.py`` trains with ``nn.Dropout``, whose masks come from torch's
generator, so with dropout on it can only be compared statistically.  Here the mask is an input: ``uniform01``
restates the hash of ``mlp::uniform01`` (alphadia_amd/csrc/adh_mlp.hip) in NumPy uint64 arithmetic, and
``masked_fit`` is the network of ``fdr_oracle._network`` written functionally, in float32 or float64:

    BatchNorm1d (batch statistics) -> [Linear -> ReLU -> mask * 1 / (1 - p)] x hidden -> Linear -> Softmax,
    binary_cross_entropy against [1 - y, y, 0, ...], torch.optim.Adam with weight decay.

The float64 run is the arbiter of tests/test_mlp_exact_gpu.py; the float32 run measures how far float32
arithmetic alone moves the result (the noise the device is allowed a multiple of).
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np


def uniform01(seed, step, row, layer, j) -> np.ndarray:
    """mlp::uniform01: a splitmix64-style hash of (seed, step, row, layer, unit) -> float32 in [0, 1) with
    24 bits.  ``row`` is the row's position inside its batch, ``step`` the global optimiser step
    (first_step + s), ``layer`` the index of the hidden Linear.  Arguments broadcast."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * (
            np.asarray(step, dtype=np.uint64) + np.uint64(1))
        z = z ^ ((np.asarray(row, dtype=np.uint64) << np.uint64(32)) | (np.asarray(layer, dtype=np.uint64) << np.uint64(24))
                 | np.asarray(j, dtype=np.uint64))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def keep_mask(seed, step, layer, n_rows: int, n_units: int, dropout: float) -> np.ndarray:
    """(n_rows, n_units) bool: True where the unit stays.  The device drops where u < float32(p)."""
    u = uniform01(seed, step, np.arange(n_rows)[:, None], layer, np.arange(n_units)[None, :])
    return ~(u < np.float32(dropout))


def split_params(dims, params):
    """The flat parameter vector of the C ABI -> gamma, beta, [(W, b) per Linear]."""
    d = dims[0]
    gamma, beta = params[:d], params[d : 2 * d]
    off, lin = 2 * d, []
    for i in range(len(dims) - 1):
        n_in, n_out = dims[i], dims[i + 1]
        w = params[off : off + n_in * n_out].reshape(n_out, n_in)
        off += n_in * n_out
        lin.append((w, params[off : off + n_out]))
        off += n_out
    assert off == len(params)
    return gamma, beta, lin


def _forward(h, lin, masks, scale, pre=None):
    import torch

    for l, (w, b) in enumerate(lin[:-1]):
        z = h @ w.T + b
        if pre is not None:
            pre.append(z.detach().numpy().copy())
        h = torch.relu(z)
        if masks is not None:
            h = h * masks[l] * scale
    w, b = lin[-1]
    return torch.softmax(h @ w.T + b, dim=1)


Fit = namedtuple("Fit", "params rm rv losses pre moments")


def masked_fit(dtype, dims, params, rm, rv, x, y, train_rows, batch_start, batch_size, lr, wd, dropout, seed=0,
               first_step=0, betas=(0.9, 0.999), eps=1e-8, bn_eps=1e-5, momentum=0.1, moments=None, threads=2) -> Fit:
    """Train on ``batch_start`` as adh_mlp_fit does; ``dtype`` is torch.float32 or torch.float64.

    Returns Fit(params, running_mean, running_var, loss per step, pre, moments): ``pre[s][l]`` is the
    (batch, units) pre-activation of hidden Linear l at step s (the ReLU knife-edge condition needs it) and
    ``moments`` the Adam state, which a continued fit (first_step > 0) takes back through ``moments=``.
    Like fdr_oracle.mlp_fit it sets torch's thread count for the whole process (``threads``, 2 as the oracle)."""
    import torch
    import torch.nn.functional as F

    torch.set_num_threads(threads)
    dims = [int(v) for v in dims]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    flat = torch.tensor(np.asarray(params).astype(npdt), requires_grad=True)
    opt = torch.optim.Adam([flat], lr=lr, weight_decay=wd, betas=betas, eps=eps)
    if first_step:
        if moments is None:
            raise ValueError("a continued fit needs the moments of the steps before it")
        opt.state[flat] = dict(step=torch.tensor(float(first_step)), exp_avg=torch.tensor(moments[0].astype(npdt)),
                               exp_avg_sq=torch.tensor(moments[1].astype(npdt)))
    xt = torch.tensor(np.asarray(x, np.float32)[train_rows].astype(npdt))
    y1 = np.asarray(y, np.float32)[train_rows].astype(npdt)
    target = np.zeros((len(y1), dims[-1]), dtype=npdt)
    target[:, 0], target[:, 1] = 1 - y1, y1
    target = torch.tensor(target)
    rm = torch.tensor(np.asarray(rm).astype(npdt))
    rv = torch.tensor(np.asarray(rv).astype(npdt))
    p32 = np.float32(dropout)
    scale = float(npdt(1) / (npdt(1) - npdt(p32)))
    B = int(batch_size)
    losses, pre = [], []
    for s, b0 in enumerate(batch_start):
        b0 = int(b0)
        xb = xt[b0 : b0 + B]
        mean, var = xb.mean(0), xb.var(0, unbiased=False)
        gamma, beta, lin = split_params(dims, flat)
        h = (xb - mean) / torch.sqrt(var + bn_eps) * gamma + beta
        masks = None
        if dropout > 0:
            masks = [torch.tensor(keep_mask(seed, first_step + s, l, B, dims[l + 1], dropout).astype(npdt))
                     for l in range(len(dims) - 2)]
        step_pre = []
        prob = _forward(h, lin, masks, scale, step_pre)
        loss = F.binary_cross_entropy(prob, target[b0 : b0 + B])
        opt.zero_grad()
        loss.backward()
        opt.step()
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * (B / (B - 1))
        losses.append(float(loss.item()))
        pre.append(step_pre)
    st = opt.state[flat]
    mom = (st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()) if st else None
    return Fit(flat.detach().numpy().copy(), rm.numpy().copy(), rv.numpy().copy(), np.asarray(losses, np.float64), pre, mom)


def eval_forward(dtype, dims, params, rm, rv, x, bn_eps=1e-5) -> np.ndarray:
    """network.eval(): running statistics, no dropout."""
    import torch

    dims = [int(v) for v in dims]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    with torch.no_grad():
        gamma, beta, lin = split_params(dims, torch.tensor(np.asarray(params).astype(npdt)))
        rm, rv = torch.tensor(np.asarray(rm).astype(npdt)), torch.tensor(np.asarray(rv).astype(npdt))
        h = (torch.tensor(np.asarray(x, np.float32).astype(npdt)) - rm) / torch.sqrt(rv + bn_eps) * gamma + beta
        return _forward(h, lin, None, 1.0).numpy()


def random_problem(seed, d, layers, output_dim=2, n=3000):
    """The generator of test_fdr._random_problem with the seed and the output width as arguments: feature
    columns of very different scale and offset, one constant column, torch's default Linear initialisation."""
    import torch

    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.5).astype(np.float32)
    x = (rng.normal(size=(n, d)) * rng.uniform(0.1, 30, d) + rng.uniform(-10, 100, d) + y[:, None] * rng.uniform(0, 8, d))
    x = x.astype(np.float32)
    x[:, 0] = 3.5  # a constant column: variance 0 in every batch
    torch.manual_seed(seed)
    dims = [d, *layers, output_dim]
    parts = [rng.uniform(0.5, 1.5, d).astype(np.float32), rng.normal(size=d).astype(np.float32) * 0.1]
    for i in range(len(dims) - 1):
        lin = torch.nn.Linear(dims[i], dims[i + 1])
        parts += [lin.weight.detach().numpy().ravel(), lin.bias.detach().numpy().ravel()]
    params = np.concatenate(parts).astype(np.float32)
    return rng, x, y, dims, params, rng.normal(size=d).astype(np.float32), rng.uniform(0.5, 2, d).astype(np.float32)


def knife_edge(fit32: Fit, fit64: Fit):
    """(smallest |pre-activation| of the float64 run, largest float32 - float64 pre-activation difference) over
    every step and hidden layer.  A unit whose pre-activation changes sign between the two changes the gradient
    by a finite amount, so an exact comparison needs the first to be well above the second."""
    zmin, err = np.inf, 0.0
    for s32, s64 in zip(fit32.pre, fit64.pre):
        for z32, z64 in zip(s32, s64):
            zmin = min(zmin, float(np.abs(z64).min()))
            err = max(err, float(np.abs(z32.astype(np.float64) - z64).max()))
    return zmin, err
