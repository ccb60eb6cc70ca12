"""The library staged from its columns and calibrated in HBM, host side: the record dtype against the header
and the path ``HipCalibrationManager.predict_staged`` takes, against a context that only records calls.
The device side is in tests/test_stage_calibrated_gpu.py."""

from __future__ import annotations

import os
import re

import numpy as np
import pandas as pd
import pytest

from alphadia_amd import _abi, runtime
from alphadia_amd import calibration as cal
from test_calibration import CASES, FITTED, golden_model, np_predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(ROOT, "include", "alphadia_hip.h")) as f:
        return f.read()


def test_record_dtype_matches_the_header_comment():
    dt = _abi.LIB_RECORD_DTYPE
    assert dt.itemsize == 32
    comment = re.search(r"/\*(?:(?!\*/).)*?Byte offsets:(.*?)\*/\s*int adh_staged_fragments_read", _header(), re.S).group(1)
    comment = " ".join(comment.replace("*", " ").split())
    offsets = {name: int(off) for name, off in re.findall(r"([a-z_]+) (\d+)(?= |,|;)", comment)}
    fields = ["mz_library", "mz", "intensity", "type", "loss_type", "charge", "number", "position", "cardinality"]
    assert set(fields) <= set(offsets), offsets
    for name in fields:
        assert dt.fields[name][1] == offsets[name], name
        assert dt.fields[name][0] == (np.float32 if offsets[name] < 12 else np.uint8), name
    assert "18 .. 31 zero" in comment
    assert dt.fields["pad"][1] == 18 and dt.fields["pad"][0].itemsize == 14


def test_record_dtype_matches_the_device_struct():
    with open(os.path.join(ROOT, "alphadia_amd", "csrc", "adh_device.h")) as f:
        body = re.search(r"struct __attribute__\(\(aligned\(16\)\)\) LibRec \{(.*?)\};", f.read(), re.S).group(1)
    size = {"float": 4, "uint8_t": 1, "uint32_t": 4}
    off, offsets = 0, {}
    for ctype, names in re.findall(r"(float|uint8_t|uint32_t) ([^;]+);", body):
        for name in names.split(","):
            name = name.strip()
            count = int(re.search(r"\[(\d+)\]", name).group(1)) if "[" in name else 1
            offsets[name.split("[")[0]] = off
            off += size[ctype] * count
    assert off == 32
    for name, (_, at) in ((k, v[:2]) for k, v in _abi.LIB_RECORD_DTYPE.fields.items() if k != "pad"):
        assert offsets[name] == at, name
    assert offsets["pad0"] == _abi.LIB_RECORD_DTYPE.fields["pad"][1]


@pytest.mark.parametrize("name", [n for n in FITTED if CASES[n]["meta"]["dtype"] == "float32"])
def test_golden_queries_stay_within_the_knife_edge_cap(name):
    """The float32 of the reference's own predictions: the rows whose rounding the last bits of a float64 could flip
    (tests/test_calibration_gpu.py: f32_knife_edge) are within the cap check_against allows, for the reference alone."""
    from test_calibration_gpu import f32_knife_edge

    c = CASES[name]
    model = golden_model(c)
    for q, want in ((c["query"], c["pred"]), (c["query_nan"], c["pred_nan"])):
        assert q.dtype == np.float32
        got, scale = np_predict(model.scale_mean, model.scale_max, model.beta, q)
        finite = ~np.isnan(want)
        assert np.array_equal(np.isnan(got), ~finite)
        bound = 1e-13 * scale[finite]
        assert (np.abs(got[finite] - want[finite]) <= bound).all()
        edge = f32_knife_edge(want[finite], bound)
        assert edge.sum() <= max(2, 1e-4 * finite.sum()), int(edge.sum())
        same = got[finite].astype(np.float32) == want[finite].astype(np.float32)
        assert (same | edge).all()


# ---------------------------------------------------------------------------------------------------------------------


class FakeContext:
    """Records what ``predict_staged`` asks of the context; the predictions are the model's intercept + the input."""

    def __init__(self, staged: bool):
        self.staged = staged
        self.calls: list[str] = []
        self.frame = None
        self.column_at_adopt = None

    def staged_from(self, *eight):
        assert len(eight) == 8
        self.calls.append("staged_from")
        return self.staged

    def _values(self, mz_library):
        return np.asarray(mz_library, dtype=np.float64) + 0.25

    def calibrate_staged_fragments(self, model):
        self.calls.append("calibrate_staged_fragments")
        return self._values(self.frame["mz_library"].to_numpy())

    def stage_fragments_calibrated(self, model, *eight):
        assert len(eight) == 8
        self.calls.append("stage_fragments_calibrated")
        return self._values(eight[0])

    def calibration_predict(self, model, x):
        self.calls.append("calibration_predict")
        return self._values(x)

    def adopt_fragment_columns(self, *nine):
        assert len(nine) == 9
        self.calls.append("adopt_fragment_columns")
        self.column_at_adopt = self.frame["mz_calibrated"].to_numpy().copy() if "mz_calibrated" in self.frame else None
        # the nine columns are the frame's own, the calibrated one in the m/z position
        assert nine[1] is not None and np.array_equal(nine[1], self.frame["mz_calibrated"].to_numpy())
        assert np.shares_memory(nine[0], self.frame["mz_library"].to_numpy())


def _frame(n=40):
    rng = np.random.default_rng(3)
    return pd.DataFrame({
        "mz_library": rng.uniform(200, 1500, n).astype(np.float32), "intensity": rng.random(n).astype(np.float32),
        "type": rng.integers(97, 123, n).astype(np.uint8), "loss_type": np.zeros(n, np.uint8),
        "charge": rng.integers(1, 3, n).astype(np.uint8), "number": rng.integers(1, 30, n).astype(np.uint8),
        "position": rng.integers(0, 30, n).astype(np.uint8), "cardinality": np.ones(n, np.uint8)})


def _manager(fitted=True):
    m = cal.HipCalibrationManager(path=None, load_from_file=False, has_ms1=True, has_mobility=False)
    if fitted:
        e = m.get_estimator("fragment", "mz")
        g = golden_model(CASES["mz_f32"])
        for k in ("scale_mean", "scale_max", "beta", "n_kernels", "polynomial_degree"):
            setattr(e.model, k, getattr(g, k))
        e.is_fitted = True
    return m


@pytest.fixture
def fake(monkeypatch):
    def install(staged):
        ctx = FakeContext(staged)
        monkeypatch.setattr(runtime, "get_context", lambda device=None: ctx)
        return ctx
    return install


@pytest.mark.parametrize("staged, only_if_staged, path, call", [
    (True, False, "in_place", "calibrate_staged_fragments"),
    (True, True, "in_place", "calibrate_staged_fragments"),
    (False, False, "staged", "stage_fragments_calibrated"),
    (False, True, "host", "calibration_predict"),
])
def test_predict_staged_path_choice(fake, staged, only_if_staged, path, call):
    ctx = fake(staged)
    df = _frame()
    ctx.frame = df
    assert _manager().predict_staged(df, only_if_staged=only_if_staged) == path
    assert call in ctx.calls
    assert df["mz_calibrated"].dtype == np.float64
    assert np.array_equal(df["mz_calibrated"].to_numpy(), df["mz_library"].to_numpy().astype(np.float64) + 0.25)
    others = {"calibrate_staged_fragments", "stage_fragments_calibrated", "calibration_predict"} - {call}
    assert not others & set(ctx.calls)
    if path == "host":
        assert "adopt_fragment_columns" not in ctx.calls
    else:
        # the column is in the frame before the columns are adopted: the key is taken from the frame's own column
        assert ctx.calls[-1] == "adopt_fragment_columns"
        assert np.array_equal(ctx.column_at_adopt, df["mz_calibrated"].to_numpy())


def test_predict_staged_not_fitted_is_skipped(fake, caplog):
    ctx = fake(True)
    df = _frame()
    ctx.frame = df
    with caplog.at_level("WARNING"):
        assert _manager(fitted=False).predict_staged(df) == "skipped"
    assert "skipped as it has not been fitted" in caplog.text
    assert "mz_calibrated" not in df.columns
    assert not {"calibrate_staged_fragments", "stage_fragments_calibrated", "adopt_fragment_columns",
                "calibration_predict"} & set(ctx.calls)


def test_only_if_staged_never_stages(fake):
    for staged in (False, True):
        ctx = fake(staged)
        df = _frame()
        ctx.frame = df
        _manager().predict_staged(df, only_if_staged=True)
        assert "stage_fragments_calibrated" not in ctx.calls


def test_predict_staged_overwrites_an_existing_column(fake):
    ctx = fake(True)
    df = _frame()
    df["mz_calibrated"] = df["mz_library"].astype(np.float64)
    ctx.frame = df
    assert _manager().predict_staged(df) == "in_place"
    assert np.array_equal(ctx.column_at_adopt, df["mz_library"].to_numpy().astype(np.float64) + 0.25)


class _HiddenManager:
    """A calibration manager without ``predict_staged`` (the reference's)."""

    def __init__(self):
        self.calls = []

    def predict(self, df, group):
        self.calls.append(group)


class _StagedManager(_HiddenManager):
    def predict_staged(self, df, group_name="fragment", device=None, only_if_staged=False):
        self.calls.append(("staged", group_name, device, only_if_staged))
        return "in_place"


def test_lock_and_requantification_prefer_predict_staged():
    from types import SimpleNamespace

    from alphadia_amd.optimization import BatchLibrary, HipOptimizationLock

    lock = HipOptimizationLock.__new__(HipOptimizationLock)
    lock._device = 3
    lock.batch_library = BatchLibrary(pd.DataFrame({"a": [1]}), pd.DataFrame({"b": [1]}))
    hidden, staged = _HiddenManager(), _StagedManager()
    lock.update_with_calibration(hidden)
    assert hidden.calls == ["precursor", "fragment"] and lock.last_fragment_calibration == "host"
    lock.update_with_calibration(staged)
    assert staged.calls == ["precursor", ("staged", "fragment", 3, True)] and lock.last_fragment_calibration == "in_place"

    from alphadia_amd import multiplexing

    seen = {}

    def stop(*a, **k):
        raise StopIteration

    orig = multiplexing.requantify_multiplexed
    multiplexing.requantify_multiplexed = stop
    try:
        for manager in (_HiddenManager(), _StagedManager()):
            library = SimpleNamespace(precursor_df_unfiltered=pd.DataFrame(), _fragment_df=pd.DataFrame(),
                                      fragment_df=pd.DataFrame())
            config = {"multiplexing": {"reference_channel": 0, "decoy_channel": 12, "target_channels": "4,8"},
                      "search": {"experimental_xic": True}}
            names = SimpleNamespace(get_rt_column=lambda: "rt", get_mobility_column=lambda: "mobility",
                                    get_precursor_mz_column=lambda: "mz", get_fragment_mz_column=lambda: "mz")
            handler = multiplexing.HipMultiplexingRequantificationHandler(
                config, manager, None, SimpleNamespace(log_string=lambda *a, **k: None), names, library, device=1)
            with pytest.raises(StopIteration):
                handler._score(None, pd.DataFrame({"channel": [0]}), resident=False)
            seen[type(manager).__name__] = manager.calls
    finally:
        multiplexing.requantify_multiplexed = orig
    assert seen["_HiddenManager"] == ["precursor", "fragment"]
    assert seen["_StagedManager"] == ["precursor", ("staged", "fragment", 1, True)]
