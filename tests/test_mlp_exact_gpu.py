"""The classifier's training kernel (alphadia_amd/csrc/adh_mlp.hip) against a float64 reference that applies the
kernel's own dropout masks (tests/mlp_reference.py), and at its limits: hidden layers wider than one round of the
8 waves, no hidden layer, up to 8 classes, the two BCELoss clamps, predict past its grid cap, scratch reuse.

The exact cases follow test_fdr.test_hip_forward_backward_match_torch_fp32: Adam with lr = 1, eps = 1 makes the
parameter change a smooth image of the gradient, so one and two steps from a set state check the whole forward
and backward pass, here with dropout on.  Every comparison is logged to mlp_exact.jsonl,
beside test_gpu_parity's parity_masks.jsonl.
"""

from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import mlp_exact_cases as E
import mlp_reference as R
from oracle import fdr_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from alphadia_amd import runtime

    return runtime.get_context(0)


def _log(record: dict) -> None:
    """One line per comparison in mlp_exact.jsonl: noise, device error and bound, printed and kept before anything
    is asserted.  The file is kept beside the suite's other comparison log, parity_masks.jsonl of test_gpu_parity
    (which runs first), in the directory that a GPU run brings back."""
    import glob

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    record = dict(test=os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], **record)
    print("[mlp_exact]", json.dumps(record))
    for beside in sorted(glob.glob(os.path.join(root, "*", "parity_masks.jsonl")))[:1]:
        try:
            with open(os.path.join(os.path.dirname(beside), "mlp_exact.jsonl"), "a") as f:
                f.write(json.dumps(record) + "\n")
        except OSError:
            pass


def _device(ctx, name):
    from alphadia_amd import runtime

    c, p = E.BY_NAME[name], E.problem(name)
    mlp = runtime.DeviceMlp(ctx, c.d, c.layers, c.output_dim)
    mlp.set_state(p.params, p.rm, p.rv)
    mlp.stage_rows(p.x, p.y)
    return mlp


def _fit(mlp, name, schedule, seed=E.MASK_SEED, first_step=0, lr=E.LR):
    c, p = E.BY_NAME[name], E.problem(name)
    return mlp.fit(p.train_rows, schedule, c.batch_size, lr, E.WD, c.dropout, seed=seed, first_step=first_step, **E.ADAM)


# ---------------------------------------------------------------------------------------------
# forward and backward, dropout on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_hip_forward_backward_exact_with_dropout(ctx, name):
    """One and two optimiser steps of adh_mlp_fit vs masked_fit(float64) with the kernel's masks.

    Bound on |delta param device - delta param float64|: max(5e-6, 16 x noise), where 5e-6 is the bound of
    test_hip_forward_backward_match_torch_fp32 for the same comparison and noise = max |delta param
    masked_fit(float32) - delta param masked_fit(float64)| comes from the two references alone; the factor 16
    covers the device's other summation order (16-row tiles, MFMA chains, 8 tile groups).  Loss to rtol 2e-6,
    running statistics to rtol 1e-5 / atol 1e-6, both against float64.  No row or unit is masked out of the
    comparison: the data seed of each case keeps every pre-activation away from zero (mlp_exact_cases.py), which is
    asserted here from the references."""
    c, r = E.BY_NAME[name], E.references(name)
    p = r.problem
    p0 = p.params.astype(np.float64)
    for f32, f64 in ((r.one32, r.one64), (r.two32, r.two64)):
        zmin, err = R.knife_edge(f32, f64)
        assert zmin > c.knife_margin * err, (zmin, err)
        assert np.abs(f64.params - p0).max() > 1e-4  # the step moved something

    mlp = _device(ctx, name)
    loss1 = _fit(mlp, name, p.schedule[:1])
    p1, rm1, rv1, nbt = mlp.get_state()
    # the second step continues the moments and the mask's step counter
    loss2 = _fit(mlp, name, p.schedule[1:], first_step=1)
    p2, rm2, rv2, nbt2 = mlp.get_state()
    mlp.close()

    rec = dict(case=name, batch_size=c.batch_size, d=c.d, layers=c.layers, output_dim=c.output_dim, dropout=c.dropout)
    checks = []
    for tag, got, f32, f64, loss, rm, rv in (("one", p1, r.one32, r.one64, loss1, rm1, rv1),
                                             ("two", p2, r.two32, r.two64, np.concatenate([loss1, loss2]), rm2, rv2)):
        noise = E.noise(f32, f64, p.params)
        bound = max(5e-6, 16 * noise)
        error = float(np.abs((got.astype(np.float64) - p0) - (f64.params - p0)).max())
        loss_rel = float(np.abs(loss.astype(np.float64) / f64.losses - 1).max())
        rec.update({f"{tag}_noise": noise, f"{tag}_error": error, f"{tag}_bound": bound, f"{tag}_loss_rel": loss_rel,
                    f"{tag}_largest_change": float(np.abs(f64.params - p0).max())})
        checks.append((error, bound, loss, f64, rm, rv))
    _log(rec)
    assert nbt == 1 and nbt2 == 2
    for error, bound, loss, f64, rm, rv in checks:
        np.testing.assert_allclose(loss, f64.losses, rtol=2e-6)
        np.testing.assert_allclose(rm, f64.rm, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rv, f64.rv, rtol=1e-5, atol=1e-6)
        assert error <= bound, (error, bound)


@pytest.mark.parametrize("name", ["production-p0.5", "9-blocks"])
def test_hip_dropout_step_counter_seed_and_eval(ctx, name):
    """With dropout 0.5: a fit in one call equals the same schedule split at k with first_step = k, bit for bit
    (the mask's step is first_step + s, not s; the schedule repeats a batch, which then has the same batch
    statistics and another mask); the mask of every step is the reference's; another seed gives other parameters
    and the same seed on a fresh object the same; predict() after the fit is the eval-mode forward, without dropout."""
    c, p = E.BY_NAME[name], E.problem(name)
    B = c.batch_size
    schedule = np.array([B, 0, B, 2 * B, 0], dtype=np.int64)
    k = 2
    mlp = _device(ctx, name)
    loss_a = _fit(mlp, name, schedule)
    state_a = mlp.get_state()
    proba = mlp.predict()

    mlp.set_state(p.params, p.rm, p.rv)
    loss_b = np.concatenate([_fit(mlp, name, schedule[:k]), _fit(mlp, name, schedule[k:], first_step=k)])
    state_b = mlp.get_state()
    np.testing.assert_array_equal(loss_b, loss_a)
    for a, b in zip(state_a[:3], state_b[:3]):
        np.testing.assert_array_equal(b, a)
    assert state_b[3] == len(schedule)

    # lr = 0 (and no weight decay through it): the parameters stay, so the loss of every step is the loss of the
    # initial network on that batch under that step's mask.  Steps 0 and 2 see the same batch.
    mlp.set_state(p.params, p.rm, p.rv)
    loss_0 = np.concatenate([_fit(mlp, name, schedule[:3], lr=0.0), _fit(mlp, name, schedule[3:], first_step=3, lr=0.0)])
    np.testing.assert_array_equal(mlp.get_state()[0], p.params)
    ref_0 = E.fit_reference(name, torch.float64, schedule, lr=0.0)
    np.testing.assert_allclose(loss_0, ref_0.losses, rtol=2e-6)
    assert abs(ref_0.losses[0] - ref_0.losses[2]) > 1e-3 * ref_0.losses[0]  # same batch, visibly another mask

    mlp.set_state(p.params, p.rm, p.rv)
    _fit(mlp, name, schedule, seed=E.MASK_SEED + 1)
    other = mlp.get_state()[0]
    assert np.abs(other - state_a[0]).max() > 1e-3
    mlp.close()

    fresh = _device(ctx, name)
    np.testing.assert_array_equal(_fit(fresh, name, schedule), loss_a)
    for a, b in zip(state_a[:3], fresh.get_state()[:3]):
        np.testing.assert_array_equal(b, a)
    fresh.close()

    # eval: the float64 forward of the fitted state (the device's own, so that only the forward is compared)
    ref = R.eval_forward(torch.float64, p.dims, state_a[0], state_a[1], state_a[2], p.x)
    np.testing.assert_allclose(proba, ref, rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------
# the two BCELoss clamps
# ---------------------------------------------------------------------------------------------
def _gaps(dims, params, x_batch):
    """float64 logit gap z1 - z0 of every row of a batch in training mode (batch statistics, no dropout)."""
    x = torch.tensor(x_batch.astype(np.float64))
    gamma, beta, lin = R.split_params(dims, torch.tensor(params.astype(np.float64)))
    h = (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + 1e-5) * gamma + beta
    for w, b in lin[:-1]:
        h = torch.relu(h @ w.T + b)
    z = h @ lin[-1][0].T + lin[-1][1]
    return (z[:, 1] - z[:, 0]).numpy()


def test_hip_bce_clamps_on_saturated_rows(ctx):
    """Rows whose logit gap exceeds 110: expf underflows to exactly 0, p is exactly {0, 1}, and half of the rows
    are on the wrong class.  Then log(p) is clamped at -100, so the loss is 100 x wrong / B, and (1 - p) p is
    clamped at 1e-12, so d loss / d logits = p_c (g_c - sum g p) is exactly 0 and the step is weight decay alone.

    The arbiter is the float32 oracle (fdr_oracle.mlp_fit): torch's float32 BCELoss has the same two clamps, and
    float64 cannot arbitrate because there exp(-110) is an ordinary number and nothing is clamped.  Rows that are
    nearly but not fully saturated (p (1 - p) between 1e-12 and ~1e-4) are not compared: there 1 - p carries an
    O(1) relative rounding error in float32 on both sides, and the two sides need not agree."""
    from alphadia_amd import runtime

    B, d, layers = 64, 5, [8]
    rng, x, y, dims, params, rm, rv = R.random_problem(5, d, layers)
    train_rows = rng.permutation(len(x))[: len(x) - 100]
    gap = _gaps(dims, params, x[train_rows[:B]])
    K = 120.0 / np.abs(gap).min()
    last = 2 * d + d * layers[0] + layers[0]  # start of the last Linear
    big = params.copy()
    big[last:] *= np.float32(K)
    gap = _gaps(dims, big, x[train_rows[:B]])
    assert np.abs(gap).min() > 110
    y = y.copy()
    wrong = np.arange(B) % 2 == 0
    y[train_rows[:B]] = np.where(wrong, gap < 0, gap > 0).astype(np.float32)
    schedule, adam = np.zeros(1, dtype=np.int64), dict(betas=(0.9, 0.999), eps=1.0)

    mlp = runtime.DeviceMlp(ctx, d, layers, 2)
    mlp.set_state(big, rm, rv)
    mlp.stage_rows(x, y)
    loss = mlp.fit(train_rows, schedule, B, 1.0, 1e-5, 0.0, **adam)
    p1 = mlp.get_state()[0]
    mlp.close()
    ref = fdr_oracle.mlp_fit(dims, big, rm, rv, x, y, train_rows, schedule, B, 1.0, 1e-5, **adam)
    _log(dict(case="bce-clamps", loss=float(loss[0]), oracle_loss=float(ref[3][0]), expected=100.0 * wrong.sum() / B,
              step_error=float(np.abs((p1 - big) - (ref[0] - big)).max())))
    assert loss[0] == pytest.approx(100.0 * wrong.sum() / B, rel=2e-6)
    assert ref[3][0] == pytest.approx(100.0 * wrong.sum() / B, rel=2e-6)
    assert np.isfinite(p1).all()
    # Adam on the gradient wd * p alone: m^ / (sqrt(v^) + 1) = wd p / (wd |p| + 1)
    wd_step = 1e-5 * big.astype(np.float64) / (1e-5 * np.abs(big.astype(np.float64)) + 1.0)
    assert (np.abs((big.astype(np.float64) - ref[0]) - wd_step) <= np.spacing(np.abs(big)) + 1e-7).all()
    np.testing.assert_allclose(p1 - big, ref[0] - big, rtol=0, atol=1e-7)


def test_hip_bce_loss_on_denormal_probabilities(ctx):
    """Rows whose logit gap is 95 ... 100: the smaller probability exp(-gap) is a float32 denormal, k = 26 ... 3900
    units of 2^-149.  Only the loss is compared, against the float32 oracle.  A device that flushed denormals would
    see p = 0 and clamp the row's log at -100: the loss would be exactly 100 x wrong / B, ~1.3 % above the oracle's.

    Tolerance: rtol 2e-6 plus, per wrong row, 1 / (k - 1) on its -log(p): the device and the oracle each round the
    same exp(-gap) to one of its two neighbouring units, so they differ by one unit at the most, and log moves by
    1 / k per unit.  k comes from the float64 gap.

    The network is built so that the gap is K x (normalised feature 1): unit 0 = relu(xn_1), unit 1 = relu(-xn_1),
    logit 1 - logit 0 = K (unit 0 - unit 1)."""
    from alphadia_amd import runtime

    B, d, layers = 64, 5, [8]
    dims = [d, *layers, 2]
    rng = np.random.default_rng(95)
    n = 200
    x = rng.normal(size=(n, d)).astype(np.float32)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    x[:, 1] = (sign * rng.uniform(95.6, 99.4, n)).astype(np.float32)
    gamma, beta = np.ones(d), np.zeros(d)
    w1, b1 = np.zeros((8, d)), np.zeros(8)
    w1[0, 1], w1[1, 1] = 1.0, -1.0
    w2, b2 = np.zeros((2, 8)), np.zeros(2)
    w2[1, 0], w2[1, 1] = 1.0, -1.0
    train_rows = np.arange(n, dtype=np.int64)
    std = np.sqrt(x[:B, 1].astype(np.float64).var() + 1e-5)
    mean = x[:B, 1].astype(np.float64).mean()
    w2 *= std  # undo the normalisation: gap = x_1 - mean
    params = np.concatenate([gamma, beta, w1.ravel(), b1, w2.ravel(), b2]).astype(np.float32)
    gap = _gaps(dims, params, x[:B])
    assert np.abs(mean) < 0.5 and 95 < np.abs(gap).min() and np.abs(gap).max() < 100
    wrong = np.arange(B) % 4 < 2  # both signs among the wrong rows
    y = np.zeros(n, dtype=np.float32)
    y[:B] = np.where(wrong, gap < 0, gap > 0)
    k = np.exp(-np.abs(gap[wrong])) / 2.0 ** -149
    assert k.min() > 20 and k.max() < 4000
    expected = (100.0 + np.abs(gap[wrong])).sum() / (2 * B)  # t = 0 on p = 1: clamped; t = 1 on p = exp(-gap)
    slack = (1.0 / (k - 1)).sum() / (2 * B)
    schedule, adam = np.zeros(1, dtype=np.int64), dict(betas=(0.9, 0.999), eps=1.0)
    rm, rv = np.zeros(d, np.float32), np.ones(d, np.float32)

    mlp = runtime.DeviceMlp(ctx, d, layers, 2)
    mlp.set_state(params, rm, rv)
    mlp.stage_rows(x, y)
    loss = float(mlp.fit(train_rows, schedule, B, 1.0, 1e-5, 0.0, **adam)[0])
    mlp.close()
    ref = float(fdr_oracle.mlp_fit(dims, params, rm, rv, x, y, train_rows, schedule, B, 1.0, 1e-5, **adam)[3][0])
    flushed = 100.0 * wrong.sum() / B
    _log(dict(case="bce-denormals", loss=loss, oracle_loss=ref, float64_loss=expected, flushed_loss=flushed, slack=slack,
              device_keeps_denormals=bool(abs(loss - flushed) > abs(loss - expected))))
    assert abs(ref - expected) <= 2e-6 * expected + slack      # the oracle keeps denormals
    assert flushed - expected > 100 * slack                     # and a flush would show
    assert abs(loss - ref) <= 2e-6 * ref + slack, (loss, ref, flushed)


# ---------------------------------------------------------------------------------------------
# predict past its grid cap, scratch reuse
# ---------------------------------------------------------------------------------------------
def test_hip_predict_past_the_grid_cap(ctx):
    """16 * 2048 + 5 rows are 2049 tiles for the 2048 workgroups of adh_mlp_predict_kernel: workgroup 0 takes a
    second tile, and that tile has 5 rows."""
    from alphadia_amd import runtime

    d, layers = 5, [8]
    n = 16 * 2048 + 5
    rng, x0, _, dims, params, rm, rv = R.random_problem(5, d, layers)
    x = np.tile(x0, (n // len(x0) + 1, 1))[:n] + rng.normal(size=(n, d)).astype(np.float32) * np.float32(0.01)
    x = x.astype(np.float32)
    ref = fdr_oracle.mlp_predict(dims, params, rm, rv, x)
    mlp = runtime.DeviceMlp(ctx, d, layers, 2)
    mlp.set_state(params, rm, rv)
    mlp.stage_rows(x)
    proba = mlp.predict()
    assert proba.shape == (n, 2)
    np.testing.assert_allclose(proba, ref, rtol=0, atol=2e-6)
    perm = rng.permutation(n)
    by_rows = mlp.predict(perm)
    np.testing.assert_allclose(by_rows, ref[perm], rtol=0, atol=2e-6)
    back = np.empty_like(by_rows)
    back[perm] = by_rows
    np.testing.assert_array_equal(back, proba)
    rep = np.concatenate([perm, rng.integers(0, n, 12)])  # 16 * 2048 + 17 rows with repeats: 2050 tiles, the last with 1 row
    rng.shuffle(rep)
    assert len(rep) == 16 * 2048 + 17
    by_rep = mlp.predict(rep)
    np.testing.assert_allclose(by_rep, ref[rep], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(by_rep, proba[rep])
    mlp.close()


def test_hip_fit_reuses_its_scratch(ctx):
    """One adh_mlp_t fitted three times from the same state, with 37 x 3, 256 x 9 and 16 x 2 (batch size x distinct
    batches): the tile gradients, loss partials, BatchNorm partials, statistics and tickets grow for the second
    fit and are reused, larger than needed, by the third.  Every fit equals a fresh object's, bit for bit."""
    from alphadia_amd import runtime

    d, layers = 12, [24, 8]
    rng, x, y, dims, params, rm, rv = R.random_problem(12, d, layers)
    train_rows = rng.permutation(len(x))[: len(x) - 100]

    def fit(mlp, B, n_distinct):
        starts = np.arange(n_distinct, dtype=np.int64) * B
        schedule = np.concatenate([starts[::-1], starts[:2]])  # unsorted, two batches twice
        mlp.set_state(params, rm, rv)
        # x_train / y_train of the call (118, 2311 and 39 rows) are device scratch too
        loss = mlp.fit(train_rows[: n_distinct * B + 7], schedule, B, 1e-3, 1e-5, 0.3, seed=E.MASK_SEED)
        return (loss, *mlp.get_state()[:3])

    reused = runtime.DeviceMlp(ctx, d, layers, 2)
    reused.stage_rows(x, y)
    for B, n_distinct in ((37, 3), (256, 9), (16, 2)):
        got = fit(reused, B, n_distinct)
        fresh = runtime.DeviceMlp(ctx, d, layers, 2)
        fresh.stage_rows(x, y)
        exp = fit(fresh, B, n_distinct)
        fresh.close()
        assert np.isfinite(got[0]).all() and np.abs(got[1] - params).max() > 1e-4
        for a, b in zip(got, exp):
            np.testing.assert_array_equal(a, b)
    reused.close()
