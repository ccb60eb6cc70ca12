/*
 * alphadia_hip_lfq.h - C ABI of label-free quantification (directLFQ) in libalphadia_hip.so, on the
 * resident fragment matrices of alphadia_hip.h's cross-run quantity object.
 *
 * Replaces QuantBuilder.direct_lfq (outputtransform/quantification/quant_builder.py:184-245).  The
 * directlfq package is not at hand: the procedure is pinned to this repository's restatement only
 * (alphadia_amd/lfq.py: host_direct_lfq), which states the published method with its
 * corner decisions written out.
 *
 * Conventions as in alphadia_hip.h: every function returns 0 or a negative error code, the message is
 * available from that header's last-error call.
 */
#ifndef ALPHADIA_HIP_LFQ_H
#define ALPHADIA_HIP_LFQ_H

#include "alphadia_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One quantification over matrix `column` of a built quantity object (n_keys x n_runs float32; v <= 0 and NaN are
 * missing, x = log2(v) in float64).  keep[n_keys]: the rows that take part (NULL: all); group[n_keys]: the group
 * code of every row, 0 .. n_groups - 1 in the order the groups are reported in (a negative code drops the row).
 * Rows in (group, row) order, rows without a value dropped; if normalize, one shift per run (runs as traces);
 * per group the ions are normalised as traces (the num_samples_quadratic fullest by pair merging, the others
 * onto their median trace), the per-run median of at least min_nonan values is scaled to the group's summed
 * intensity, missing runs give 0, a group without any run is dropped.  n_kept: the groups reported.
 */
int adlfq_run(adh_quant_t *quant, int32_t column, const uint8_t *keep, const int32_t *group, int32_t n_groups,
              int32_t min_nonan, int32_t num_samples_quadratic, int32_t normalize, int64_t *n_kept);
/* the last run's result: group[n_kept] codes in ascending order and table[n_kept x n_runs] float64, row-major */
int adlfq_result(adh_quant_t *quant, int32_t *group, double *table);
/* HIP-event times (ms) of the last run: prepare, sample normalisation (with its host control), group kernels */
int adlfq_time_ms(adh_quant_t *quant, double *prepare_ms, double *sample_ms, double *group_ms);

#ifdef __cplusplus
}
#endif

#endif /* ALPHADIA_HIP_LFQ_H */
