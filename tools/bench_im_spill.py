"""Spill instantiation of the ion-mobility feature kernel against its LDS launch groups: HIP-event time of the feature
launches of a call on input A of tests/box_sweep_im_oversize.py (98 rows with 200-fragment slices, own layouts up to
160 544 bytes), once and in 30 copies, every row through each instantiation (ADH_DEBUG_IM_DYNAMIC_LAYOUT, with and
without ADH_DEBUG_IM_SPILL).  Prints one JSON line (profiles/im_oversize.json, `spill_vs_lds`).

    python tools/bench_im_spill.py
"""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the synthetic data generators live with the tests
import box_sweep_im_oversize as bo  # noqa: E402
from alphadia_amd import runtime  # noqa: E402
from alphadia_amd.scoring import fragment_columns, pack_assembled  # noqa: E402

SWITCHES = ("ADH_DEBUG_IM_DYNAMIC_LAYOUT", "ADH_DEBUG_IM_SPILL")


def main():
    ctx = runtime.get_context(0)
    case, soa, spec = bo.ragged()
    ctx.stage_run(case.dia, force=True)
    ctx.stage_fragments(*fragment_columns(case.library.fragment_df, "mz_library"), force=True)
    out = {}
    for copies in (1, 30):
        rows = np.tile(np.arange(len(spec)), copies)
        m = pack_assembled(bo.rows_of(soa, rows))
        for name in ("all_fragments", "no_xic_all_fragments"):
            cfg = bo.config_of(name, "A").to_jitclass()
            res = {}
            for label, on in (("lds_groups", SWITCHES[:1]), ("spill", SWITCHES)):
                for k in SWITCHES:
                    os.environ.pop(k, None)
                os.environ.update({k: "1" for k in on})
                for _ in range(2):
                    ctx.score_host(m, cfg)
                times = []
                for _ in range(7):
                    ctx.kernel_time_ms(reset=True)
                    ctx.im_launch_stats(reset=True)
                    ctx.score_host(m, cfg)
                    _, feature_ms, launches = ctx.kernel_time_ms(reset=True)
                    times.append(feature_ms * launches)
                stats = ctx.im_launch_stats(reset=True)
                res[label] = {"feature_ms_median": float(np.median(times)), "feature_ms_min": float(min(times)),
                              "feature_ms_max": float(max(times)), "candidates_per_group": stats["candidates"].tolist(),
                              "lds_bytes_per_group": stats["lds_bytes"].tolist()}
            res["ratio_spill_over_lds"] = res["spill"]["feature_ms_median"] / res["lds_groups"]["feature_ms_median"]
            out[f"{name}_x{copies}"] = dict(rows=len(rows), **res)
    for k in SWITCHES:
        os.environ.pop(k, None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
