/*
 * alphadia_hip_flatten.h - C ABI of the device flatten in libalphadia_hip.so: the dense library (a precursor table
 * plus two row-aligned float32 matrices) in, the flat fragment table out, optionally left staged on the handle as
 * the LibRec records alphadia_hip.h's column staging would have made of it.
 *
 * Replaces FlattenLibrary (alphabase's calc_fragment_cardinality + SpecLibFlat.parse_base_library).  alphabase is
 * not at hand: the rules are pinned to this repository's restatement only (alphadia_amd/flatten.py:
 * host_flatten_library), which writes every corner decision out.
 *
 * Conventions as in alphadia_hip.h: every function returns 0 or a negative error code, the message is
 * available from that header's last-error call.
 */
#ifndef ALPHADIA_HIP_FLATTEN_H
#define ALPHADIA_HIP_FLATTEN_H

#include "alphadia_hip.h"

/* limits of the input: columns of the matrices, rows of one precursor's block, precursors of one group */
#define ADFL_MAX_COLUMNS 32
#define ADFL_MAX_ROWS 255
#define ADFL_MAX_GROUP 255
/* route bounds: a group of up to this many precursors has its cardinalities counted by one wavefront, a larger one
 * by a workgroup; a block of up to this many cells (rows x columns) is ranked by one wavefront in its LDS tile, a
 * larger one by a workgroup.  ADFL_DEBUG_ROUTE=block sends everything to the workgroups; ADFL_DEBUG_ROUTE=wave
 * sends every group of up to ADFL_CARD_WAVE_DEBUG_MEMBERS precursors to a wavefront (the tile bound stays). */
#define ADFL_CARD_WAVE_MAX_MEMBERS 16
#define ADFL_CARD_WAVE_DEBUG_MEMBERS 64
#define ADFL_SELECT_WAVE_MAX_CELLS 320

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One flatten.  Precursor p owns the dense rows [frag_start[p], frag_stop[p]) of mz / intensity (n_rows x n_cols,
 * row-major): 0 .. ADFL_MAX_ROWS rows inside the matrices, blocks of different precursors disjoint (checked on the
 * device on the blocks ordered by (start, row count)).  Its group is (decoy[p], elution_group[p]); decoy may be NULL,
 * elution_group lies in [0, 2^56).  column_codes[4 x n_cols]: type, loss_type, charge, counts-from-the-N-terminus
 * of every column.
 *
 * cardinality of a cell: 1 + the other precursors of the group with |mz_q - mz_p| < 1e-5 in the same cell, where
 * every precursor of the group has the same row count (else 1; a NaN difference does not count); a group of more
 * than ADFL_MAX_GROUP precursors is refused.  Kept: intensity > min_intensity and among the top_k of the block by
 * (intensity, flat index) descending; NaN is never kept, -0 ties with +0.  Kept cells come out in dense flat order:
 * out_mz / out_intensity [capacity], out_bytes[6 x capacity] (type, loss_type, charge, number, position,
 * cardinality, each column `capacity` apart), flat_start / flat_stop[n_prec] in the caller's row order.  capacity
 * must hold the kept rows (the sum over the precursors of min(top_k, cells) always does); n_flat: how many there are.
 *
 * stage != 0: the records (mz = mz_library = the cell's m/z) are left staged on the handle, device and host mirror,
 * as adh_stage_fragments_columns over the returned columns would leave them.  A refused input leaves the staged
 * library as it was.
 *
 * routes[4]: groups counted by a wavefront / by a workgroup, blocks ranked by a wavefront / by a workgroup;
 * kernel_ms: HIP-event time of the sorts, scans and kernels; link_bytes[2]: bytes host -> device, device -> host.
 */
int adfl_flatten(adh_handle_t *h, int64_t n_prec, const int64_t *frag_start, const int64_t *frag_stop,
                 const int64_t *elution_group, const uint8_t *decoy, int64_t n_rows, int32_t n_cols, const float *mz,
                 const float *intensity, const uint8_t *column_codes, int32_t top_k, float min_intensity, int32_t stage,
                 int64_t capacity, uint32_t *flat_start, uint32_t *flat_stop, float *out_mz, float *out_intensity,
                 uint8_t *out_bytes, int64_t *n_flat, int64_t *routes, double *kernel_ms, uint64_t *link_bytes);

#ifdef __cplusplus
}
#endif

#endif /* ALPHADIA_HIP_FLATTEN_H */
