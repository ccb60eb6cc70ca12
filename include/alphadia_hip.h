/*
 * alphadia_hip.h - C ABI of libalphadia_hip.so, the MI355X-native drop-in for
 * alphaDIA's peptide-centric candidate scoring hot path.
 *
 * Nothing like this exists in the reference (it is pure Python + Numba); each
 * entry point below names the reference interface whose work it replaces.
 * All paths are relative to the MannLabs/alphadia source tree.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types cross this ABI
 *   - every function returns ADH_OK (0) or a negative error code; the message
 *     is available from adh_last_error() (thread local)
 *   - per-candidate soft failures are DATA (valid[i] == 0), never errors,
 *     exactly like `Candidate.failed` (search/scoring/containers/candidate.py:190-325)
 *   - host buffers are owned by the caller; device buffers live behind the
 *     opaque handle until adh_destroy()
 *   - a handle is bound to one GPU and is not re-entrant (one host thread per GPU)
 */
#ifndef ALPHADIA_HIP_H
#define ALPHADIA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADH_OK 0
#define ADH_ERR_INVALID_ARGUMENT (-1)
#define ADH_ERR_HIP (-2)
#define ADH_ERR_NOT_STAGED (-3)
#define ADH_ERR_UNSUPPORTED (-4)
#define ADH_ERR_OUT_OF_MEMORY (-5)

#define ADH_NUM_FEATURES 46 /* alphadia/constants/settings.py:5 */

/* candidate flag bits */
#define ADH_FLAG_SKIP 1u /* score group without its reference channel: score_group.py:50-64 */

/*
 * Raw data of a non-ion-mobility run: the fields of AlphaRawJIT
 * (search/jitclasses/alpharaw_jit.py:78-138) that the scoring path reads.
 * Peaks are CSR by spectrum, m/z ascending inside each spectrum.
 */
typedef struct adh_alpharaw {
    const double *cycle;            /* (1, cycle_len, cycle_scans, 2) float64, C order */
    int32_t cycle_len;              /* cycle.shape[1] */
    int32_t cycle_scans;            /* cycle.shape[2] (1 for AlphaRaw) */
    const float *rt_values;         /* [n_spectra] seconds */
    int64_t n_spectra;
    const float *mobility_values;   /* [n_mobility]; {1e-6, 0} for AlphaRaw */
    int64_t n_mobility;
    const int64_t *peak_start_idx;  /* [n_spectra] */
    const int64_t *peak_stop_idx;   /* [n_spectra] */
    const float *mz_values;         /* [n_peaks] */
    const float *intensity_values;  /* [n_peaks] */
    int64_t n_peaks;
} adh_alpharaw_t;

/*
 * Raw data of an ion-mobility run in the transposed (TOF-major) layout: the fields of
 * TimsTOFTransposeJIT (search/jitclasses/bruker_jit.py:22-137) that the scoring path reads.
 * push index = frame * scan_max_index + scan; events are ascending in push inside a TOF bin.
 */
typedef struct adh_timstof {
    const double *cycle;                /* (1, cycle_len, scan_max_index, 2) float64 */
    int32_t cycle_len;
    int32_t scan_max_index;
    const int64_t *dia_precursor_cycle; /* [cycle_len * scan_max_index] cycle row of a push */
    const double *rt_values;            /* [n_frames] */
    int64_t n_frames;
    const double *mobility_values;      /* [scan_max_index] */
    const double *mz_values;            /* [n_tof] m/z of a TOF index, ascending */
    int64_t n_tof;
    const int64_t *tof_indptr;          /* [n_tof + 1] */
    const uint32_t *push_indices;       /* [n_events] */
    const uint16_t *intensity_values;   /* [n_events] */
    int64_t n_events;
    int32_t zeroth_frame;               /* 1 when frame 0 is the empty alphatims frame */
} adh_timstof_t;

/*
 * Flat fragment library: the nine arrays of FragmentContainer
 * (search/jitclasses/fragment_container.py:11-46) as assembled by
 * CandidateScoring.assemble_fragments (search/scoring/scoring.py:355-392).
 */
typedef struct adh_fragments {
    int64_t n;
    const float *mz_library;
    const float *mz;          /* the configured fragment m/z column (library or calibrated) */
    const float *intensity;
    const uint8_t *type;
    const uint8_t *loss_type;
    const uint8_t *charge;
    const uint8_t *number;
    const uint8_t *position;
    const uint8_t *cardinality;
} adh_fragments_t;

/*
 * Candidate table in struct-of-arrays form: the columns
 * ScoreGroupContainer.build_from_df receives
 * (search/scoring/containers/score_group.py:145-229), already in
 * score-group order; row i of every output belongs to candidate i.
 */
typedef struct adh_candidates {
    int64_t n;
    const uint32_t *precursor_idx;
    const uint8_t *rank;
    const uint8_t *flags;            /* ADH_FLAG_* or NULL */
    const uint32_t *frag_start_idx;
    const uint32_t *frag_stop_idx;
    const int64_t *scan_start;
    const int64_t *scan_stop;
    const int64_t *scan_center;
    const int64_t *frame_start;
    const int64_t *frame_stop;
    const int64_t *frame_center;
    const uint8_t *charge;
    const float *precursor_mz;
    const float *isotope_intensity;  /* [n, n_isotope_cols] row major */
    int32_t n_isotope_cols;
} adh_candidates_t;

/* CandidateScoringConfigJIT (search/scoring/config.py:13-60) */
typedef struct adh_scoring_config {
    int32_t collect_fragments;
    int32_t score_grouped;
    int32_t exclude_shared_ions;
    uint32_t top_k_fragments;
    uint32_t top_k_isotopes;
    int32_t reference_channel;
    uint32_t quant_window;
    int32_t quant_all;
    float precursor_mz_tolerance;
    float fragment_mz_tolerance;
    int32_t experimental_xic;
    /* SimpleQuadrupoleJit.sigma / .delta_mu (search/scoring/quadrupole.py:72-76,110-113): the quadrupole
     * transfer function of a fitted calibration, logistic(x, lower + delta_mu[0], sigma[0]) -
     * logistic(x, upper + delta_mu[1], sigma[1]).  sigma[0] <= 0 (a zeroed struct) stands for the class
     * defaults the reference workflow runs with: sigma 0.2, delta_mu 0. */
    double quadrupole_sigma[2];
    double quadrupole_delta_mu[2];
} adh_scoring_config_t;

/*
 * OutputPsmDF (search/scoring/output.py:17-70): `valid`, `precursor_idx`,
 * `rank`, `features[n,46]` and thirteen per-fragment tables [n, top_k].
 * Buffers must be zero-initialised by the caller for the *_device entry
 * point; the host entry point zero-fills them itself.
 */
typedef struct adh_output {
    int64_t n;
    int32_t top_k;
    uint8_t *valid;
    uint32_t *precursor_idx;
    uint8_t *rank;
    float *features;               /* [n, 46] */
    uint32_t *fragment_precursor_idx;
    uint8_t *fragment_rank;
    float *fragment_mz_library;
    float *fragment_mz;
    float *fragment_mz_observed;
    float *fragment_height;
    float *fragment_intensity;
    float *fragment_mass_error;
    float *fragment_correlation;
    uint8_t *fragment_position;
    uint8_t *fragment_number;
    uint8_t *fragment_type;
    uint8_t *fragment_charge;
    uint8_t *fragment_loss_type;
    uint32_t *stat_matched_peaks;  /* optional [n]: peaks accumulated by get_dense, or NULL */
    /* optional [n, top_k], or NULL: 1 + position of the slot's fragment inside the candidate's library
     * slice [frag_start_idx, frag_stop_idx), 0 for an empty slot.  With it the library columns of the
     * fragment tables (mz_library, mz, position, number, type, charge, loss_type) can be rebuilt from
     * the staged library, so they need not travel in the all-gather (alphadia_amd/distributed.py). */
    uint16_t *fragment_lib_slot;
} adh_output_t;

typedef struct adh_handle adh_handle_t;

/* Thread-local message of the last failing call. */
const char *adh_last_error(void);

/* Number of visible HIP devices. */
int adh_device_count(int *count);

/* Create / destroy a per-GPU context. */
int adh_create(adh_handle_t **handle, int device);
int adh_destroy(adh_handle_t *handle);

/*
 * Stage the run in HBM once (replaces DiaData.to_jitclass(),
 * raw_data/alpharaw_wrapper.py:124-142, as consumed at scoring.py:639).
 * The run is kept as a time-major transposed copy (sorted by cycle block, cycle
 * row, m/z bin, cycle, m/z) that replaces the reference's per-spectrum binary
 * search (alpharaw_jit.py:53-64,293-297): the XIC of a fragment is contiguous.
 */
int adh_stage_alpharaw(adh_handle_t *handle, const adh_alpharaw_t *dia);

/*
 * Stage an ion-mobility run (replaces TimsTOFTranspose.to_jitclass(),
 * raw_data/bruker.py:119-152).  A handle holds ONE run: staging either layout
 * replaces the previous one.
 */
int adh_stage_timstof(adh_handle_t *handle, const adh_timstof_t *dia);

/* Stage the flat fragment library (replaces assemble_fragments, scoring.py:355-392).  Besides the copy in HBM
 * (32 bytes per fragment) the handle keeps a host copy of the packed records (another 32 bytes per fragment of
 * host memory, per handle = per rank): adh_score_candidates rebuilds the library columns of the fragment tables
 * from it on the host instead of copying them over PCIe.  ADH_DEBUG_COPY_ALL=1 does without the rebuild. */
int adh_stage_fragments(adh_handle_t *handle, const adh_fragments_t *fragments);

/*
 * Score candidates: host table in, host OutputPsmDF out (upload + kernels +
 * download).  Replaces the pjit loop `_process_score_groups`
 * (scoring.py:114-137,634-643), i.e. ScoreGroup.process -> Candidate.process
 * for every candidate.  `out` buffers are zero-filled by the call.
 * How the tables cross PCIe is a matter of policy (INTEGRATION.md lists every switch): tables of
 * ADH_COMPACT_MIN_ROWS rows and more send the filled fragment slots as one packed block per chunk
 * (ADH_COMPACT_COPY_OUT=1 / =0 forces that on / off), and in such a block tables of ADH_SPARSE_SLOTS_MIN_ROWS
 * rows and more (default 1 000 000) send fragment_intensity and fragment_correlation as streams of their non-zero
 * words (ADH_SPARSE_SLOTS=1 / =0 forces that on / off).  The caller's tables hold the same bytes either way.
 */
int adh_score_candidates(adh_handle_t *handle, const adh_candidates_t *candidates,
                         const adh_scoring_config_t *config, adh_output_t *out);

/*
 * The same call for the DataFrame operator: only what `collect_candidates` / `collect_fragments`
 * (search/scoring/scoring.py:394-467,520-580; output.py:89-97) keep of the padded tables comes back - the VALID
 * candidates (`valid`), column by column, and the FILLED fragment slots (`fragment_mz_library > 0`), in the order
 * the padded tables hold them.  Per chunk of the pipeline the device counts and scans, a pack kernel writes the
 * compacted columns - features transposed to [feature][row], library columns of a slot from the staged library -
 * densely into a device block, ONE DMA copy of exactly the used bytes moves the block into a page-locked twin of the
 * handle, and host threads unpack finished blocks into the caller's arrays (which may be pageable) while later
 * chunks are scored.  No padded host table, no host pass over invalid rows or empty slots: 1.11 GB instead of
 * 1.35 GB cross PCIe per 3 M candidates and the DataFrame operator takes 85 ms instead of 150.
 *
 * Capacities: `rows_capacity` >= number of valid candidates, `slots_capacity` >= number of filled slots
 * (candidates and candidates * top_k always suffice).  A call that would overflow either writes nothing beyond
 * them, sets n_rows / n_slots to what it needs and fails with ADH_ERR_INVALID_ARGUMENT.
 * The padded device tables are left in HBM as by adh_score_candidates (adh_get_device_tables, the FDR stage).
 */
typedef struct adh_compact_output {
    int64_t rows_capacity;          /* in */
    int64_t slots_capacity;         /* in */
    int32_t top_k;                  /* in: fragment slots per candidate (width of the padded tables) */
    int32_t reserved;
    int64_t n_rows;                 /* out: valid candidates */
    int64_t n_slots;                /* out: filled fragment slots */
    /* per valid candidate, ascending candidate row */
    uint32_t *row;                  /* [rows_capacity] row of the candidate in adh_candidates_t */
    uint32_t *precursor_idx;        /* [rows_capacity] */
    uint8_t *rank;                  /* [rows_capacity] */
    float *features;                /* [46][rows_capacity]: feature f of the j-th valid candidate at f * rows_capacity + j */
    /* per filled fragment slot, ascending (candidate row, slot) */
    uint32_t *fragment_row;         /* [slots_capacity] row of the slot's candidate in adh_candidates_t */
    uint32_t *fragment_precursor_idx;
    uint8_t *fragment_rank;
    float *fragment_mz_library;
    float *fragment_mz;
    float *fragment_mz_observed;
    float *fragment_height;
    float *fragment_intensity;
    float *fragment_mass_error;
    float *fragment_correlation;
    uint8_t *fragment_position;
    uint8_t *fragment_number;
    uint8_t *fragment_type;
    uint8_t *fragment_charge;
    uint8_t *fragment_loss_type;
} adh_compact_output_t;

int adh_score_candidates_compact(adh_handle_t *handle, const adh_candidates_t *candidates,
                                 const adh_scoring_config_t *config, adh_compact_output_t *out);

/*
 * The same work split so that tables can stay in HBM:
 *   adh_upload_candidates  - copy the candidate SoA to the GPU (kept in the handle)
 *   adh_score_uploaded     - enqueue the kernels on `hip_stream` (a hipStream_t taken
 *                            literally: NULL is HIP's default stream; use
 *                            adh_get_stream for the handle's own stream) writing into
 *                            DEVICE buffers `out_device` (zero-initialised by the
 *                            caller ON THAT STREAM, on the handle's GPU); does not
 *                            synchronise.
 * Used when the per-GPU tables are reassembled with an RCCL all-gather before
 * they leave HBM.
 */
int adh_upload_candidates(adh_handle_t *handle, const adh_candidates_t *candidates);
int adh_score_uploaded(adh_handle_t *handle, const adh_scoring_config_t *config,
                       adh_output_t *out_device, void *hip_stream);

/*
 * Device view of the tables the last adh_score_candidates call filled (they stay in HBM until the
 * next call): the hand-over to a following on-device stage (classifier, q-values, fragment
 * competition; alphadia/workflow/peptidecentric/peptidecentric.py:219-243 hands DataFrames over
 * on the host).  device_view->n is the number of live rows.
 */
int adh_get_device_tables(adh_handle_t *handle, adh_output_t *device_view);

/*
 * Resident extraction (alphadia/workflow/peptidecentric/peptidecentric.py:183-263 on one GPU): score into the
 * handle's own padded tables and copy nothing to the host (the D2H counter of adh_transfer_counters does not move).
 * Afterwards the tables are what adh_score_candidates leaves - adh_get_device_tables, adh_fdr_resident and
 * adh_take_rows work on them; their width is top_k_fragments clamped to the longest library slice of the table, as
 * the callers of adh_score_candidates choose it.  Fails with ADH_ERR_UNSUPPORTED while a communicator is attached
 * (the tables are then a rank's shard plus a gather).
 */
int adh_score_candidates_resident(adh_handle_t *handle, const adh_candidates_t *candidates,
                                  const adh_scoring_config_t *config);

/*
 * The listed rows of the current device tables, in the layout of adh_score_candidates_compact: the VALID rows among
 * rows[0, n) in list order (a row listed twice comes back twice; invalid rows are skipped), features as
 * [46][rows_capacity], and their filled fragment slots in (list position, slot) order.  `row` and `fragment_row`
 * are table rows.  out->top_k must be the width of the device tables.  A count kernel over the listed rows, an
 * exclusive scan, a pack kernel writing one dense block and ONE copy of its used bytes; every column travels.
 * Errors: a row outside [0, rows of the tables) -> ADH_ERR_INVALID_ARGUMENT; no scored tables, or a run / library
 * staged since they were scored -> ADH_ERR_NOT_STAGED; capacities too small -> n_rows / n_slots say what is
 * needed and the call fails with ADH_ERR_INVALID_ARGUMENT, as the compact entry does.
 */
int adh_take_rows(adh_handle_t *handle, const int64_t *rows, int64_t n, adh_compact_output_t *out);

/*
 * Accumulated resident tables (the optimisation lock of alphadia/workflow/optimizers/optimization_lock.py: every step
 * scores one more batch and runs the FDR stage over all rows since the last reset).  Scores `candidates` as
 * adh_score_candidates_resident does and puts their rows behind the rows already accumulated: row i of an earlier
 * batch stays row i, and *first_row is the row of the batch's first candidate.  Afterwards the device tables
 * (adh_get_device_tables, adh_fdr_resident, adh_take_rows, adh_resident_counts) hold rows [0, n) of every batch since
 * the last reset, with the width of the widest batch (narrower rows have zeroed slots behind theirs: byte for byte
 * the tables one adh_score_candidates_resident call over all the batches leaves).  Each row keeps the library values
 * of the time it was scored; staging another library or run afterwards leaves the accumulated tables readable.  A
 * batch that needs more rows or wider slots moves the rows in HBM into a new layout; capacity grows geometrically.
 * Any other scoring call, and adh_resident_reset, ends the accumulation; a failed append ends it too.  Fails with
 * ADH_ERR_UNSUPPORTED while a communicator is attached.
 */
int adh_score_candidates_resident_append(adh_handle_t *handle, const adh_candidates_t *candidates,
                                         const adh_scoring_config_t *config, int64_t *first_row);

/* empty the device tables (the next adh_score_candidates_resident_append starts at row 0); keeps the memory */
int adh_resident_reset(adh_handle_t *handle);

/*
 * The valid rows of the current device tables and their filled fragment slots: the row counts of the features and
 * fragments frames the tables stand for.  A count kernel over rows [0, n) and a 16-byte copy.  Errors as adh_take_rows.
 */
int adh_resident_counts(adh_handle_t *handle, int64_t *valid_rows, int64_t *filled_slots);

/*
 * Layout of the packed device buffer that holds the tables of `rows` candidates (the buffer
 * adh_get_device_tables / adh_comm_gathered give views of): one entry per OutputPsmDF column
 * (alphadia/search/scoring/output.py:17-97) in buffer order, every table 256-byte aligned.  The computed
 * tables come first and form the contiguous "wire" prefix of `wire_bytes` bytes - what the all-gather of
 * adh_comm_init and the D2H copies of adh_score_candidates move; the columns behind it (wire = 0) repeat the
 * candidate table or the staged library and are rebuilt where they are needed.  Pure function: needs no
 * GPU.  fields may be NULL to query n_fields / the sizes only.
 */
typedef struct adh_table_field {
    char name[40];
    uint64_t offset;      /* bytes from the start of the buffer */
    uint32_t row_elems;   /* elements per candidate row: 1, 46 or top_k */
    uint32_t elem_bytes;
    int32_t wire;
    int32_t reserved;
} adh_table_field_t;
int adh_table_layout(int64_t rows, int32_t top_k, int32_t capacity, adh_table_field_t *fields, int32_t *n_fields,
                     uint64_t *total_bytes, uint64_t *wire_bytes);
/* zero those tables on `hip_stream` (for callers that refill them with adh_score_uploaded) */
int adh_zero_device_tables(adh_handle_t *handle, void *hip_stream);

/*
 * Page-locked host memory for candidate columns and output tables: with it the H2D / D2H copies
 * of adh_score_candidates run asynchronously at full PCIe rate and overlap the kernels.  Pageable
 * buffers are accepted everywhere, they are just slower.
 */
int adh_host_alloc(void **ptr, uint64_t bytes);
/* blocking copy of `bytes` bytes from a device pointer of one of the views above to host memory */
int adh_copy_to_host(adh_handle_t *handle, void *dst, const void *src_device, uint64_t bytes);
int adh_host_free(void *ptr);

/*
 * Device buffers of 256 MB and more that the library no longer needs (sort temporaries of a staging call, tables and
 * scratch it outgrew, what a destroyed handle held) are parked and reused instead of freed - freeing gigabytes of
 * device memory leaves the runtime's DMA copies at half the link rate for the rest of the process.  This
 * call returns everything parked (at most ADH_DEV_CACHE_GB, default 48) to the runtime.
 */
int adh_trim_device_cache(void);

/*
 * How many host threads a scoring call over a table of n_rows candidates starts for its host-side work (rebuilding the
 * id / library columns behind the copy-out, unpacking the compact blocks), and the CPU budget that number is cut from:
 * the smallest of the hardware threads, the scheduler affinity mask and the cgroup CPU quota (cpu.max), divided by
 * LOCAL_WORLD_SIZE - the ranks of a node share one quota -, at most 16, a thread per 16 384 rows at least;
 * ADH_HOST_THREADS overrides it.  Replaces the `thread_count` argument of CandidateScoring.__call__
 * (alphadia/search/scoring/scoring.py:583-661, `alphatims.utils.set_threads`), which the reference leaves to the caller.
 * Needs no GPU.  Either pointer may be NULL.
 */
int adh_host_threads(int64_t n_rows, int32_t *threads, int32_t *cpu_budget);

/*
 * The chunk boundaries of a host -> host scoring call over n_rows > 0 candidates: chunk i of the pipeline is rows
 * [cuts[i], cuts[i + 1]), cuts[0] = 0, cuts[*n_cuts - 1] = n_rows.  ion_mobility: the staged run is an ion-mobility run;
 * max_rows > 0: no chunk longer than that (the call passes the fit of the ion-mobility scratch and the 32-bit offsets of
 * the compacted copy-outs), 0: no bound; packed: the call uses the compacted copy-out of the padded tables (a short
 * last chunk).  Reads ADH_CHUNK, ADH_CHUNK_PARTS, ADH_CHUNK_MIN, ADH_FIRST_CHUNK_DIV and ADH_LAST_CHUNK_DIV as the call
 * does.  *n_cuts is set even where `capacity` entries are too few (ADH_ERR_INVALID_ARGUMENT then).  Needs no GPU.
 */
int adh_chunk_cuts(int64_t n_rows, int32_t ion_mobility, int64_t max_rows, int32_t packed, int64_t *cuts, int64_t capacity,
                   int64_t *n_cuts);

/*
 * dst[i] = src[idx[i]] for n entries of arrays of CPython object pointers (NumPy dtype=object) - the string columns
 * the features frame takes over from the precursor table (scoring.py:430-445 merges them in) - on `threads` host
 * threads, reference counts raised atomically.  The caller must hold the GIL for the whole call (ctypes.PyDLL) and
 * pass a fresh dst - every entry NULL or `fill` (np.empty fills an object array with references to None; they are
 * given back); idx outside [0, n_src) fails.  Host helper of the Python operator: no GPU involved.
 */
int adh_host_take_objects(void **dst, void *const *src, const int64_t *idx, int64_t n, int64_t n_src, void *fill,
                          int32_t threads);

/*
 * Test entry: the dense tile the gather kernels build for ONE query, i.e. what
 * AlphaRawJIT.get_dense (search/jitclasses/alpharaw_jit.py:208-337) /
 * TimsTOFTransposeJIT.get_dense (search/jitclasses/bruker_jit.py:273-504) return with
 * absolute_masses=True: dense[2][n_query][O][S][F] (intensity plane, then m/z plane; S = 1 for an
 * AlphaRaw run, whose two scan slots are copies, alpharaw_jit.py:326-333) and the cycle rows
 * (`precursor_idx_list`) in obs[0..*n_obs).  mz_query must be ascending (ADH_ERR_INVALID_ARGUMENT
 * otherwise: the kernels sort by m/z, get_dense does not).  Runs the production
 * gather kernel on a one-candidate plan built from the query.
 */
int adh_debug_get_dense(adh_handle_t *handle, int64_t frame_start, int64_t frame_stop, int64_t scan_start,
                        int64_t scan_stop, const float *mz_query, int32_t n_query, float mass_tolerance,
                        float quad_lo, float quad_hi, float *dense, int64_t dense_capacity, int32_t *obs,
                        int32_t *n_obs, int32_t *n_scans, int32_t *n_cycles);

/*
 * Test entry: the table-driven log of candidate selection (csrc/adh_log_f32.h) on n host values, as the
 * library's build compiles it.  out64[i] is the float64 log of x[i] for 1 <= x[i] < inf and NaN elsewhere;
 * out32[i] is what the two smoothing kernels store by their three-way dispatch: 0 for x[i] == 1, the rounded
 * table log inside [1, inf), the library routine's float32 log for everything else (below 1, NaN, +inf).
 * lds_table != 0: every workgroup copies the table to LDS first and reads it there, as the ion-mobility
 * smoothing kernel does.  n == 0 returns without a launch.
 */
int adh_debug_log_f32(adh_handle_t *handle, const float *x, int64_t n, int32_t lds_table, double *out64,
                      float *out32);

/*
 * Test entry: the same log over every float32 bit pattern in [first_bits, last_bits], which must lie inside
 * [0x3F800000, 0x7F7FFFFF] (1 <= x < inf), in one launch, against the device library's float64 log of the
 * same argument.  *n_mismatch: arguments whose two logs round to different float32 values (never truncated);
 * mismatch_bits[0 .. min(*n_mismatch, capacity)): their bit patterns, ascending when all of them fit;
 * *max_ulps, *max_bits: the largest |table log - library log| in units of the library value's spacing, and
 * the smallest argument that reaches it.
 */
int adh_debug_log_f32_sweep(adh_handle_t *handle, uint32_t first_bits, uint32_t last_bits, int32_t lds_table,
                            int64_t *n_mismatch, uint32_t *mismatch_bits, int64_t capacity, double *max_ulps,
                            uint32_t *max_bits);

/* The handle's own (non-blocking) stream as a hipStream_t. */
int adh_get_stream(adh_handle_t *handle, void **hip_stream);

/* Block until all work enqueued on the handle's stream has finished. */
int adh_synchronize(adh_handle_t *handle);

/*
 * Average durations (milliseconds per adh_score_uploaded call) of the two scoring
 * kernels since the last reset, measured with HIP events on the launch stream:
 * `gather_ms` = fragment selection + XIC gather, `feature_ms` = the feature stack.
 */
int adh_kernel_time_ms(adh_handle_t *handle, double *gather_ms, double *feature_ms,
                       int64_t *launches, int reset);

/*
 * Candidates per kernel class (`counts[37]`) of every plan whose scoring kernels were launched on the
 * handle since the last reset, summed over the chunks of all scoring entry points.  Read-only host
 * counters: tests pin the routing with them.  Classes of an AlphaRaw plan, in processing order:
 *    0 ..  6  fused gather + feature kernel, one observation, FM = 8, 12, ..., 32 cycle registers
 *    7 .. 13  the same for two observations
 *   14 .. 16  register kernels for two observations (FM = 16, 24, 32) behind the gather kernel: shapes
 *             the fused kernel does not take (more than 12 fragments kept, library slices beyond 64)
 *   17 .. 23  register kernels for one observation (FM = 8 ... 32) behind the gather kernel, likewise
 *   24 .. 26  the 64-lane register kernels (FM = 16, 24, 32), two observations, 33 ... 64 fragments kept
 *   27 .. 29  the same for one observation
 *   30 .. 32  the 32-lane register kernels, two observations, 17 ... 32 fragments kept
 *   33 .. 35  the same for one observation
 *   36        the generic LDS kernel behind the gather kernel (also rows flagged to be skipped)
 * Ion-mobility plans use classes 0 (one observation), 1 (two), 2 (one observation, small tile) and 36.
 */
int adh_plan_class_counts(adh_handle_t *handle, int64_t *counts, int32_t reset);

/*
 * Launch groups of the generic class (36) of an AlphaRaw plan.  Its candidates are launched in three groups
 * by the LDS layout each one needs on its own (fragments kept x observations x cycles):
 *   group 0  layouts up to 38 784 bytes (several blocks share a CU)
 *   group 1  layouts up to 161 664 bytes (160 KiB less the kernel's 2 176 bytes of static LDS)
 *   group 2  larger ones: the spill instantiation, with the [K][O][F] tile planes in the scratch slab
 * `stats[0..2]`: candidates per group of every plan whose generic kernels were launched on the handle since
 * the last reset, summed over chunks and entry points; `stats[3..5]`: the largest dynamic LDS (bytes) any such
 * launch of the group asked for.  Read-only host counters: tests prove with them which path ran.
 * ADH_DEBUG_GENERIC_SPILL (set to any value) sends every generic candidate to group 2.
 */
#define ADH_GENERIC_LAUNCH_STATS 6
int adh_generic_launch_stats(adh_handle_t *handle, int64_t *stats, int32_t reset);

/*
 * Launch groups of the dynamic route of an ion-mobility plan: the launches of the feature kernel whose blocks lay
 * their LDS out at run time (a plan class whose maxima no fixed layout holds; every class with
 * ADH_DEBUG_IM_DYNAMIC_LAYOUT set).  Inside its class a candidate is launched in one of three groups by the LDS
 * layout it needs on its own (fragments kept x observations x (scans + cycles)):
 *   group 0  layouts up to 38 784 bytes (several blocks share a CU)
 *   group 1  layouts up to 161 280 bytes (160 KiB less the kernel's 2 560 bytes of static LDS)
 *   group 2  larger ones: the spill instantiation, with the work and profile regions in the scratch slab
 * `stats[0..2]`: candidates per group of every plan whose launches took the dynamic route on the handle since the
 * last reset, summed over classes, chunks and entry points; `stats[3..5]`: the largest dynamic LDS (bytes) any
 * such launch of the group asked for.  Nothing is counted for a refused call.
 * ADH_DEBUG_IM_SPILL (set to any value) sends every candidate of the dynamic route to group 2.
 */
#define ADH_IM_LAUNCH_STATS 6
int adh_im_launch_stats(adh_handle_t *handle, int64_t *stats, int32_t reset);

/*
 * The route every plan class of an ion-mobility launch takes: the rule the launches themselves follow, as a call of
 * its own.  In: the launch maxima - fragments kept k, observations o, scans s, cycles f - and the isotopes i of the
 * call, the candidates per plan class (`n_class[37]`, the classes of adh_plan_class_counts) and the scoring config.
 * Reads the ADH_DEBUG_IM* launch switches as a launch does.  Out, per plan class (`layout[37]`, `launch[37]`; both 0
 * for a class without candidates):
 *   layout  the capacities of the feature kernel: fixed at compile time for small tiles (1), for the common shape
 *           with one observation (2) or two (3), or every block with its candidate's own (4: the dynamic route, whose
 *           launch groups adh_im_launch_stats counts)
 *   launch  tile and profile phase in one kernel with four candidates per wavefront (1), the tile phase so and then
 *           the profile kernel (2), one candidate per wavefront and then the profile kernel (3), the one-kernel path (4)
 * Every route computes the same bits: tests use this call to know which routes their inputs reach.  Needs no GPU.
 */
#define ADH_IM_LAYOUT_NONE 0
#define ADH_IM_LAYOUT_SMALL 1
#define ADH_IM_LAYOUT_COMMON 2
#define ADH_IM_LAYOUT_COMMON2 3
#define ADH_IM_LAYOUT_DYNAMIC 4
#define ADH_IM_LAUNCH_NONE 0
#define ADH_IM_LAUNCH_FUSED4 1
#define ADH_IM_LAUNCH_TILE4 2
#define ADH_IM_LAUNCH_SPLIT1 3
#define ADH_IM_LAUNCH_ONE 4
int adh_im_launch_routes(int32_t k, int32_t o, int32_t s, int32_t f, int32_t i, const int64_t *n_class,
                         const adh_scoring_config_t *config, int32_t *layout, int32_t *launch);

/* ------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, candidates sharded by contiguous score-group ranges
 * (score groups are independent, search/scoring/containers/score_group.py:66-75), ONE RCCL
 * all-gather of the computed tables over xGMI.  librccl is loaded on first use.
 * ---------------------------------------------------------------------- */

/* 128-byte RCCL unique id (rank 0 creates it; the caller hands it to every rank). */
int adh_comm_unique_id(void *id128);
/*
 * Attach a communicator to the handle.  From now on every adh_score_candidates call lays its
 * device tables out for `max_rows_per_rank` rows (the largest shard, so that all ranks agree on the
 * layout) and, once its kernels are enqueued, all-gathers the computed tables of all ranks into
 * HBM on a stream of its own.  The call returns when the host tables are complete; the gather may
 * still run and overlaps the next call (two table slots).  adh_comm_wait blocks until it is done.
 */
int adh_comm_init(adh_handle_t *handle, int rank, int world, const void *id128, int64_t max_rows_per_rank);
int adh_comm_destroy(adh_handle_t *handle);
int adh_comm_wait(adh_handle_t *handle);
/* Device view of rank `rank`'s computed tables after the last call's gather (waits for it). */
int adh_comm_gathered(adh_handle_t *handle, int rank, adh_output_t *device_view, int64_t *rows);
/* max over ranks of *value (in place); also the barrier of the benchmark.  No-op without a communicator. */
int adh_comm_all_reduce_max(adh_handle_t *handle, double *value);
int adh_comm_barrier(adh_handle_t *handle);
/* Every rank passes `bytes` bytes of host memory (the same count on all ranks) and receives world x bytes in
 * rank order (recv holds world x bytes; without a communicator recv = send).  The exchange of the two other
 * stages of the path that shard without touching each other's rows - candidate selection by precursor range
 * (selection.py:620-660) and fragment competition by DIA window (fragcomp/fragcomp.py:204-229,278): one gather
 * of the per-rank results (alphadia_amd/selection.py, alphadia_amd/fragcomp.py).  The reference runs both on
 * the threads of one process and has no counterpart. */
int adh_comm_all_gather_host(adh_handle_t *handle, const void *send, uint64_t bytes, void *recv);
/* What RCCL itself reports for the attached communicator (ncclCommUserRank / ncclCommCount): rank 0 of 1
 * without one.  bench.py prints it, so that a run on N GPUs shows that N ranks met. */
int adh_comm_info(adh_handle_t *handle, int *rank, int *world);
/* hipDeviceSynchronize on the handle's GPU. */
int adh_device_synchronize(adh_handle_t *handle);

/*
 * Fragment competition inside one run (replaces `_compete_for_fragments`,
 * fragcomp/fragcomp.py:51-143).  PSMs are sorted by (window, proba, precursor)
 * and windows are given as [start, stop) row ranges exactly as
 * FragmentCompetition.__call__ prepares them (fragcomp.py:268-289); the row ranges of
 * different windows must not overlap.  valid[] is input/output (all ones on entry; a PSM
 * that enters with 0 neither removes nor is looked at, as in the reference's loops).
 */
int adh_fragcomp(adh_handle_t *handle, int64_t n_windows, const int64_t *window_start,
                 const int64_t *window_stop, int64_t n_psm, const float *rt,
                 const int64_t *frag_start_idx, const int64_t *frag_stop_idx,
                 int64_t n_frag, const float *fragment_mz, double rt_tol_seconds,
                 double mass_tol_ppm, uint8_t *valid);
/*
 * FragmentCompetition.__call__ (fragcomp/fragcomp.py:204-299) from the columns of its two frames: the preparation the
 * reference does with pandas - candidate keys (fragcomp/utils.py:48-58), the fragment range of every PSM
 * (add_frag_start_stop_idx, utils.py:11-45; PSMs without fragment rows leave), the DIA window of every PSM
 * (_add_window_idx, fragcomp.py:170-202; `window_lower` / `window_upper` = per cycle row the lowest / highest isolation
 * limit over its scans), the processing order (window, proba, precursor_idx, input position) - runs on the device, then
 * the competition.  Out: `rows[0 .. *n_rows)` = input position of every processed PSM in processing order, `valid` its
 * flag.  `*grouped` = 0 (and nothing else done) when a candidate's fragment rows are not contiguous in the fragment
 * table or a table has 2^31 rows or more: the caller then prepares the plan itself and calls adh_fragcomp.
 */
int adh_fragcomp_frames(adh_handle_t *handle, int64_t n_psm, const uint32_t *psm_precursor_idx, const uint8_t *psm_rank,
                        const float *psm_mz_observed, const float *psm_rt_observed, const float *psm_proba, int64_t n_frag,
                        const uint32_t *frag_precursor_idx, const uint8_t *frag_rank, const float *frag_mz_observed,
                        int32_t n_cycle_rows, const double *window_lower, const double *window_upper, double rt_tol_seconds,
                        double mass_tol_ppm, int64_t *rows, uint8_t *valid, int64_t *n_rows, int32_t *grouped);

/* What the last competition on this handle (adh_fragcomp or inside adh_fdr_resident) did: HIP-event
 * duration of its device work, (PSM, RT neighbour) pairs whose fragment lists were compared, PSMs whose
 * fate hung on an earlier PSM, rounds that settled those, and whether the one-workgroup-per-window
 * kernel had to run (the neighbour bitmap did not fit).  Any pointer may be NULL.  No reference
 * counterpart (the reference times `_compete_for_fragments` with its logger, fragcomp.py:283-289). */
int adh_fragcomp_stats(adh_handle_t *handle, double *kernel_ms, int64_t *pairs, int64_t *waiting,
                       int32_t *rounds, int32_t *serial);

/* ------------------------------------------------------------------------
 * Candidate selection - the step before scoring.
 * Non-ion-mobility (AlphaRaw) runs.
 * ---------------------------------------------------------------------- */

/*
 * Precursor table of the selection step: the columns of PrecursorFlatContainer
 * (search/selection/config_df.py; filled by
 * CandidateSelection._assemble_precursor_container, selection.py:712-737),
 * sorted by precursor_idx.
 */
typedef struct adh_precursors {
    int64_t n;
    const uint32_t *precursor_idx;
    const uint32_t *frag_start_idx;
    const uint32_t *frag_stop_idx;
    const uint8_t *charge;
    const float *rt;                 /* the configured rt column, seconds */
    const float *mobility;           /* unused for AlphaRaw runs */
    const float *mz;                 /* the configured precursor m/z column */
    const float *isotope_intensity;  /* [n][n_isotope_cols], row-major (columns i_0, i_1, ...) */
    int32_t n_isotope_cols;
} adh_precursors_t;

/* CandidateSelectionConfigJIT (search/selection/config_df.py:15-110), single score feature. */
typedef struct adh_selection_config {
    double rt_tolerance;
    double precursor_mz_tolerance;
    double fragment_mz_tolerance;
    int64_t candidate_count;
    int64_t top_k_precursors;        /* isotopes used */
    int64_t kernel_size;
    double f_mobility, f_rt, center_fraction;
    int64_t min_size_mobility, min_size_rt, max_size_mobility, max_size_rt;
    double join_close_candidates_scan_threshold;
    double join_close_candidates_cycle_threshold;
    double feature_mean, feature_std, feature_weight;  /* used when use_weighted_score */
    uint8_t exclude_shared_ions;
    uint8_t use_weighted_score;
    uint8_t join_close_candidates;
    uint8_t pad0;
    uint8_t pad1[4];
    double mobility_tolerance;       /* ion-mobility runs only */
} adh_selection_config_t;

/*
 * CandidateContainer (search/selection/config_df.py:227-254): n = precursors x
 * candidate_count rows, row (i * candidate_count + rank); rows that hold no
 * candidate keep score = 0 (candidate_container_to_df drops them, :270-298).
 */
typedef struct adh_candidate_table {
    int64_t n;
    uint32_t *precursor_idx;
    uint8_t *rank;
    float *score;
    uint32_t *scan_center, *scan_start, *scan_stop;
    uint32_t *frame_center, *frame_start, *frame_stop;
} adh_candidate_table_t;

/*
 * Select up to candidate_count (rt) boxes per precursor on the staged AlphaRaw
 * run and fragment library.  Replaces the pjit loop `_select_candidates_pjit`
 * (search/selection/selection.py:78-203): dense XICs of isotopes and fragments
 * over rt +- rt_tolerance, circular convolution with `kernel`
 * (GaussianKernel.get_dense_matrix, selection/kernel.py:141-218; the reference
 * does it by FFT, selection/fft.py:119-212), log-sum score, peak picking and
 * symmetric limits (selection/utils.py:46-312).  Host buffers in and out; `out`
 * is zero-filled by the call.  ADH_ERR_UNSUPPORTED, before anything is launched,
 * when more than 16 cycle rows are MS1 rows or overlap the isotope range of one
 * precursor (the kernel sums at most 16 rows per group, the reference all).
 */
int adh_select_candidates(adh_handle_t *handle, const adh_precursors_t *precursors,
                          const adh_selection_config_t *config, const float *kernel,
                          int32_t kernel_rows, int32_t kernel_cols, adh_candidate_table_t *out);

/*
 * Transpose timsTOF detector events from the frame-major alphatims layout (rows = pushes:
 * push_indptr[n_push + 1], tof_indices[n], values[n]) into the TOF-major layout the scoring and
 * selection operators read (tof_indptr[n_tof + 1], push_indices[n], values[n]; pushes ascending
 * inside a TOF bin).  Drop-in for `_transpose` (alphadia/raw_data/bruker.py:201-280), which does
 * this on 20 CPU threads when a run is loaded.  Host buffers in and out; n < 2^31.
 */
int adh_transpose_timstof(adh_handle_t *handle, const uint32_t *tof_indices, const int64_t *push_indptr,
                          int64_t n_push, int64_t n_tof, const uint16_t *values, int64_t n_events,
                          uint32_t *push_indices_out, int64_t *tof_indptr_out, uint16_t *values_out);

/* Duration (ms, HIP events) of the selection kernel of the last adh_select_candidates call. */
int adh_select_time_ms(adh_handle_t *handle, double *kernel_ms);

/* ------------------------------------------------------------------------
 * Selection -> scoring hand-over in HBM (adh_select_handover.hip): the candidate table never visits the host.
 * ---------------------------------------------------------------------- */

/*
 * adh_select_candidates without the host table: the same kernels, and the table (precursors x candidate_count rows,
 * row p * candidate_count + slot) stays in the handle's selection slab with the precursor columns and the three
 * per-precursor id columns scoring orders and groups by - the dtypes scoring.assemble_candidates converts them to.
 * Nothing is copied out.  The slab stays as it is until the next selection call; staging a run or a library ends
 * the selection.  ADH_ERR_UNSUPPORTED with a communicator attached.
 */
int adh_select_candidates_resident(adh_handle_t *handle, const adh_precursors_t *precursors,
                                   const adh_selection_config_t *config, const float *kernel, int32_t kernel_rows,
                                   int32_t kernel_cols, const uint32_t *elution_group_idx, const uint8_t *decoy,
                                   const uint8_t *channel);

/*
 * candidate_container_to_df (config_df.py:270-298), "filter 1" of the extraction handler
 * (extraction_handler.py:177-203) and scoring.assemble_candidates on the table of adh_select_candidates_resident, on
 * the device.  A row is kept when score > 0 and, with apply_cutoff, score > score_cutoff - compared in float64, so
 * the caller rounds the cutoff to the dtype NumPy compares a float32 column with it in.  The kept rows, in
 * (precursor, slot) order, are checked for (elution_group_idx, decoy, rank, precursor_idx) order and, where they are
 * not in it, brought into the order of np.lexsort((precursor_idx, rank, decoy, elution_group_idx)) by stable radix
 * passes.  score_group_idx is the row number, or with score_grouped the running count of (elution_group_idx, decoy,
 * rank) changes; a precursor_idx twice in a row of one group is ADH_ERR_INVALID_ARGUMENT ("precursor_idx must be unique
 * within a score group").  With reference_channel >= 0 the rows of groups without a row of that channel get
 * ADH_FLAG_SKIP.  One gather kernel writes the candidate columns of adh_upload_candidates into the handle's candidate
 * slab.  n_selected: rows with score > 0; n_kept: rows of the assembled table; was_sorted: 1 when no sort ran.  May be
 * called again on the same selection (another cutoff).  ADH_ERR_NOT_STAGED without a resident selection.
 */
int adh_assemble_selected(adh_handle_t *handle, int32_t apply_cutoff, double score_cutoff, int32_t score_grouped,
                          int32_t reference_channel, int64_t *n_selected, int64_t *n_kept, int32_t *was_sorted);

/* What the last adh_assemble_selected did: stats[4] = was_sorted, radix passes, score-group scans, rows flagged
 * ADH_FLAG_SKIP; assemble_ms (may be NULL): HIP-event time from its first kernel to its last. */
int adh_select_handover_stats(adh_handle_t *handle, int32_t *stats, double *assemble_ms);

/*
 * adh_score_candidates_resident on the table adh_assemble_selected left in the candidate slab: the same plan build,
 * kernel classes and device tables, nothing uploaded and nothing copied back.  ADH_ERR_NOT_STAGED when that table is
 * gone (another scoring or staging call since), ADH_ERR_UNSUPPORTED with a communicator attached.
 */
int adh_score_selected_resident(adh_handle_t *handle, const adh_scoring_config_t *config);

/* Per row of the assembled table, in its order: the row in the selection table (precursor row = table_row /
 * candidate_count) and the rank.  n must be n_kept.  5 bytes per row cross PCIe. */
int adh_selected_ids(adh_handle_t *handle, uint32_t *table_row, uint8_t *rank, int64_t n);

/*
 * The nine candidate columns of the listed rows of the assembled table (out->n == n), in list order, and - where
 * selected_pos is not NULL - the position of each among the rows with score > 0 (the index label the host's frame
 * gives it).  Errors as adh_take_rows: a row outside the table is ADH_ERR_INVALID_ARGUMENT, no assembled table
 * ADH_ERR_NOT_STAGED.
 */
int adh_take_selected(adh_handle_t *handle, const int64_t *rows, int64_t n, adh_candidate_table_t *out,
                      uint32_t *selected_pos);

/* ------------------------------------------------------------------------------------------
 * FDR stage: alphadia/fdr/fdr.py + alphadia/fdr/classifiers.py.
 * ------------------------------------------------------------------------------------------ */

/*
 * q-values of n rows.  Replaces `get_q_values` + `_fdr_to_q_values` (fdr/fdr.py:215-297): rows are
 * ordered by (score, decoy, tiebreak) ascending (stable; NaN scores last), fdr = cumulative decoys /
 * cumulative targets (float64, 1/0 = inf as in numpy), q = running minimum of fdr from the back.
 * `order_out[i]` = input row at sorted position i, `qval_out[i]` = its q-value (sorted order, as
 * the reference returns the frame).  `tiebreak` (the reference's precursor_idx) may be NULL.
 */
int adh_fdr_q_values(adh_handle_t *handle, int64_t n, const double *score, const uint8_t *decoy,
                     const int64_t *tiebreak, int64_t *order_out, double *qval_out);

/*
 * Best row per group.  Replaces `keep_best` (fdr/fdr.py:181-213): of the rows sharing
 * (group_a[, group_b]) the one with the LOWEST score stays (score = decoy probability), the
 * earliest row on ties; keep[i] = 1 for the rows that stay, rows keep their input order.
 */
int adh_fdr_keep_best(adh_handle_t *handle, int64_t n, const double *score, const int64_t *group_a,
                      const int64_t *group_b, uint8_t *keep);

/*
 * The target/decoy classifier: BatchNorm1d -> (Linear -> ReLU -> Dropout) x hidden -> Linear ->
 * Softmax trained with BCELoss and Adam (`FeedForwardNN`, fdr/classifiers.py:497-532;
 * `BinaryClassifierLegacyNewBatching.fit/predict_proba`, :316-495).  The feature matrix is staged
 * once and stays in HBM; a training step is three kernels (batch statistics, fused
 * forward/backward per 16-row tile, gradient reduction + Adam) with no host round trip.
 */
#define ADH_MLP_MAX_LINEAR 8
typedef struct adh_mlp adh_mlp_t;

typedef struct adh_mlp_arch {
    int32_t n_linear;                       /* Linear layers: hidden layers + the output layer */
    int32_t dims[ADH_MLP_MAX_LINEAR + 1];   /* input_dim, hidden sizes ..., output_dim */
    float bn_eps, bn_momentum;              /* torch.nn.BatchNorm1d defaults: 1e-5, 0.1 */
} adh_mlp_arch_t;

typedef struct adh_mlp_fit {
    const int64_t *train_rows;   /* rows of the staged matrix in training order (x_train) */
    int64_t n_train;
    const int64_t *batch_start;  /* per optimiser step: first position of its batch in train_rows */
    int64_t n_steps;
    int32_t batch_size;
    float learning_rate, weight_decay, dropout;
    float beta1, beta2, eps;     /* torch.optim.Adam defaults: 0.9, 0.999, 1e-8 */
    uint64_t seed;               /* dropout masks */
    int64_t first_step;          /* optimiser steps taken before this call; 0 resets the Adam moments */
} adh_mlp_fit_t;

int adh_mlp_create(adh_handle_t *handle, const adh_mlp_arch_t *arch, adh_mlp_t **mlp);
int adh_mlp_destroy(adh_mlp_t *mlp);
/* floats in the trainable parameter vector: bn weight[d], bn bias[d], then per Linear weight[out][in], bias[out] */
int adh_mlp_param_count(const adh_mlp_arch_t *arch, int64_t *n_params);
int adh_mlp_set_state(adh_mlp_t *mlp, const float *params, const float *running_mean, const float *running_var,
                      int64_t num_batches_tracked);
int adh_mlp_get_state(adh_mlp_t *mlp, float *params, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked);
/* copy x[n][d] (row-major float32) and, if not NULL, the class-1 target of every row to HBM */
int adh_mlp_stage_rows(adh_mlp_t *mlp, const float *x, int64_t n, int32_t d, const float *y);
/* n_steps training steps (network.train() semantics); train_loss[n_steps] may be NULL */
int adh_mlp_fit(adh_mlp_t *mlp, const adh_mlp_fit_t *fit, float *train_loss);
/* network.eval() forward of `rows` (NULL = all staged rows): proba[n][output_dim] */
int adh_mlp_predict(adh_mlp_t *mlp, const int64_t *rows, int64_t n, float *proba);
/* HIP-event time (ms) of the kernels of the last adh_mlp_fit / adh_mlp_predict call */
int adh_mlp_time_ms(adh_mlp_t *mlp, double *fit_ms, double *predict_ms);

/* ------------------------------------------------------------------------------------------
 * The FDR stage fed from the scoring tables that adh_score_candidates left in HBM: the 46-float
 * feature rows and the fragment tables never cross PCIe between scoring and FDR
 * (the reference hands DataFrames over on the host: workflow/peptidecentric/peptidecentric.py:219-243
 * -> fdr/fdr.py:24-178).  Only row-sized metadata travels.
 * ------------------------------------------------------------------------------------------ */

/*
 * Classifier rows straight from the device tables (fdr.py:86-105): of the `n_rows` candidate rows of
 * the last adh_score_candidates call, those that are valid and have no NaN in a classifier column are
 * staged, targets first, then decoys, each in row order (np.concatenate([targets, decoys])).
 * Column j of the network input is, by src_cols[j]:  0..45 = that feature;  46 + e = extra_cols[e]
 * (host float[n_rows], e.g. mz_library);  -(1 + e) = rt_observed - extra_cols[e] (delta_rt,
 * scoring.py:458).  `decoy` is a host uint8[n_rows].  Returns the staged counts.
 */
int adh_mlp_stage_rows_device(adh_mlp_t *mlp, const int32_t *src_cols, int32_t d, const float *const *extra_cols,
                              int32_t n_extra, const uint8_t *decoy, int64_t n_rows, int64_t *n_targets,
                              int64_t *n_decoys);
/*
 * The same for one part of a channel-wise decoy strategy of FDRManager.fit_predict
 * (alphadia/workflow/managers/fdr_manager.py:178-223).  `channel` is a host int64[n_rows]; row i takes part iff
 * channel[i] == target_channel || channel[i] == decoy_channel (a decoy_channel of -1 matches nothing) and it is usable
 * as above (the NaN check sees the part's rows only).  Its label is channel[i] == decoy_channel when label_by_channel
 * is set ("channel", :213-214) and decoy[i] != 0 otherwise ("precursor_channel_wise", :189-190).  Staged order, X, Y,
 * row map and decoy bytes are those of adh_mlp_stage_rows_device for that label vector; the entries after staging
 * (adh_mlp_fit, adh_mlp_predict_resident, adh_fdr_resident) do not know the difference, and a part may be staged
 * after adh_fdr_resident ran on the same tables.
 */
int adh_mlp_stage_rows_device_part(adh_mlp_t *mlp, const int32_t *src_cols, int32_t d, const float *const *extra_cols,
                                   int32_t n_extra, const uint8_t *decoy, int64_t n_rows, const int64_t *channel,
                                   int64_t target_channel, int64_t decoy_channel, int32_t label_by_channel,
                                   int64_t *n_targets, int64_t *n_decoys);
/* candidate row of every staged row (8 bytes per row; the host needs it to label its metrics) */
int adh_mlp_staged_rows(adh_mlp_t *mlp, int64_t *rows_out, int64_t capacity);
/* network.eval() forward of all staged rows; the probabilities stay in HBM */
int adh_mlp_predict_resident(adh_mlp_t *mlp);
/*
 * fdr.py:134-178 on the device: q-values of the staged rows (sorted by proba, decoy, tiebreak) ->
 * if `cycle` is given (float64 [cycle_len][cycle_scans][2], cycle_scans <= 2): the rows below
 * `fdr_heuristic` compete for fragments (fragcomp/fragcomp.py:231-299; fragment m/z from the
 * fragment_mz_observed table, rt / m/z from features 2 / 10), the others are dropped -> best row per
 * (group_a[, group_b]) -> q-values.  group_a / group_b / tiebreak are host int64[n_rows of the
 * device tables] (e.g. elution_group_idx, channel, precursor_idx).  Out (host, capacity = staged
 * rows): candidate row, class-1 probability and q-value of the surviving PSMs in the final order.
 */
int adh_fdr_resident(adh_handle_t *handle, adh_mlp_t *mlp, const int64_t *group_a, const int64_t *group_b,
                     const int64_t *tiebreak, const double *cycle, int32_t cycle_len, int32_t cycle_scans,
                     double rt_tol_seconds, double mass_tol_ppm, double fdr_heuristic, int64_t *n_out,
                     int64_t *row_out, float *proba_out, double *qval_out);
/* bytes this library has copied device -> host on the handle's GPU since the last reset */
int adh_transfer_counters(adh_handle_t *handle, uint64_t *d2h_bytes, int reset);

/* ------------------------------------------------------------------------------------------
 * Calibration of the spectral library (alphadia/workflow/managers/calibration_manager.py:34-297):
 * the prediction of a fitted LOESS model over a library column.  The fit stays on the host
 * (alphadia_amd/calibration.py): it sees a few thousand rows.
 * ------------------------------------------------------------------------------------------ */

#define ADH_LOESS_MAX_KERNELS 32
#define ADH_LOESS_MAX_DEGREE 4
#define ADH_CALIBRATION_CHUNK_ROWS (1 << 20) /* rows per pipeline chunk of adh_calibration_predict */

/* The fitted parameters of LOESSRegression (alphadia/calibration/models.py:24-366). */
typedef struct adh_loess_model {
    int32_t n_kernels;                       /* 1 .. ADH_LOESS_MAX_KERNELS */
    int32_t degree;                          /* polynomial_degree, 0 .. ADH_LOESS_MAX_DEGREE */
    double scale_mean[ADH_LOESS_MAX_KERNELS];  /* [n_kernels] kernel centres */
    double scale_max[ADH_LOESS_MAX_KERNELS];   /* [n_kernels] kernel half widths */
    double beta[(ADH_LOESS_MAX_DEGREE + 1) * ADH_LOESS_MAX_KERNELS];  /* beta[d * n_kernels + k] = NumPy's beta[d, k] */
} adh_loess_model_t;

/*
 * y[i] = LOESSRegression.predict(x)[i] (models.py:276-300, weights :302-366) for n rows of a float32
 * (x_is_f64 = 0) or float64 column: tricubic kernel weights of (x - scale_mean) / scale_max, the first kernel
 * left-open, the last right-open, normalised by their sum; y = sum_k w_k sum_d x^d beta[d, k].  The design row x^d
 * is built in the input's dtype as sklearn's PolynomialFeatures does, all else in float64.  NaN inputs and rows
 * whose weights sum to 0 give NaN, as in NumPy.  Host -> host: chunks of ADH_CALIBRATION_CHUNK_ROWS rows go
 * through two page-locked slots of the handle on two of its streams, so that the host copies of one chunk overlap
 * the transfers and kernel of the other.  Replaces the prediction the reference runs on the host for the batch
 * library of every optimisation step (workflow/managers/optimization_lock.py:148-163) and for the whole library
 * afterwards (workflow/peptidecentric/peptidecentric.py:175-180).  n may be 0.
 */
int adh_calibration_predict(adh_handle_t *handle, const adh_loess_model_t *model, const void *x, int32_t x_is_f64,
                            int64_t n, double *y);
/* Summed HIP-event duration (ms) of the kernels of the last adh_calibration_predict, adh_calibrate_staged_fragments,
 * adh_stage_fragments_columns or adh_stage_candidate_library call. */
int adh_calibration_time_ms(adh_handle_t *handle, double *kernel_ms);

/*
 * Calibrate the staged fragment library where it lies: for every record i, mz = float32 (round to nearest even) of
 * the model over its mz_library (a float32 column: x_is_f64 = 0 above), the same row evaluation as
 * adh_calibration_predict.  Only that field is written, in HBM and in the host copy of the records; nothing is
 * uploaded.  mz_out (may be NULL) receives the n float64 predictions, through the page-locked slots of
 * adh_calibration_predict and counted by adh_transfer_counters as there.  The library changes, so the call settles
 * what adh_stage_fragments settles: the last call's device tables are completed first and stop being current
 * (accumulated resident tables keep the values they were scored with), an uploaded candidate table is dropped.
 * Errors: no staged library -> ADH_ERR_NOT_STAGED; the model limits of adh_calibration_predict.  An empty library
 * is fine.
 */
int adh_calibrate_staged_fragments(adh_handle_t *handle, const adh_loess_model_t *model, double *mz_out);

/*
 * adh_stage_fragments from the nine columns without the host pack loop: the columns go up as columns (14 or 18
 * bytes per row) in chunks of ADH_CALIBRATION_CHUNK_ROWS rows through two page-locked slots, a kernel builds the
 * 32-byte records in HBM (pad bytes zero), the host team (adh_host_threads) builds the identical host copy.
 * model == NULL: fragments->mz is copied.  model != NULL: fragments->mz may be NULL and is ignored, mz is the
 * calibrated value as adh_calibrate_staged_fragments computes it from mz_library, and mz_out (may be NULL) receives
 * the float64 predictions.  Same limits, errors and effects on the handle as adh_stage_fragments.
 */
int adh_stage_fragments_columns(adh_handle_t *handle, const adh_fragments_t *fragments, const adh_loess_model_t *model,
                                double *mz_out);

/*
 * The candidate library of transfer-library requantification (_build_candidate_speclib_flat,
 * workflow/peptidecentric/transfer_library_requantification_handler.py:140-240), built in HBM from the identified
 * precursors themselves: sequence bytes, modification lists and the mass tables go up (a few dozen bytes per
 * precursor), a kernel writes the records of all fragment series at every position.  Strings stay with the caller.
 */
#define ADH_CANDIDATE_LIBRARY_MAX_SERIES 64
typedef struct adh_candidate_library {
    int64_t n;                        /* precursors */
    const int64_t *seq_offset;        /* [n + 1] into residues; L = nAA = the difference */
    const uint8_t *residues;          /* ASCII, every byte < 128 */
    const int64_t *mod_offset;        /* [n + 1] into mod_site / mod_mass, in list order */
    const int32_t *mod_site;          /* 0: residue 0 (N-terminal), -1: residue L-1 (C-terminal), s >= 1: residue s-1 */
    const double *mod_mass;
    const double *aa_mass;            /* [128] mass of a residue byte */
    double mass_proton;
    double mass_h2o;
    int32_t n_series;                 /* 1 .. ADH_CANDIDATE_LIBRARY_MAX_SERIES charged fragment types, in column order */
    const uint8_t *series_type;       /* [n_series] code point of the letter: 98 'b', 121 'y' */
    const uint8_t *series_from_nterm; /* [n_series] 1: the ion holds the N-terminus (a, b, c), 0: the C-terminus (x, y, z) */
    const uint8_t *series_charge;     /* [n_series] */
} adh_candidate_library_t;

/*
 * Precursor p with L residues: m[j] = aa_mass[residue j] plus the masses of its modifications in list order;
 * B[i] = m[0] + ... + m[i] in float64, summed left to right (np.cumsum); pep = B[L-1] + mass_h2o; Y[i] = pep - B[i].
 * It owns (L-1) * n_series consecutive rows, position-major: row i * n_series + s has
 * mz_library = float32((from_nterm ? B[i] : Y[i]) / charge_s + mass_proton), intensity 1, type series_type[s],
 * loss_type 0, charge series_charge[s], number = from_nterm ? i+1 : L-1-i, position i, cardinality 0.
 * flat_frag_start_idx / flat_frag_stop_idx [n]: the exclusive scan of the row counts in input order.  model != NULL:
 * mz = float32 of the model over mz_library, the row evaluation of adh_calibrate_staged_fragments, and mz_out (may be
 * NULL) receives the float64 predictions; model == NULL: mz = mz_library and mz_out is not written.  mz_library_out
 * (may be NULL) receives the float32 column.  Both have one entry per row.
 * ADH_ERR_INVALID_ARGUMENT, before anything is staged or written: L < 2, L > 255 (number and position are uint8), a
 * residue byte >= 128, a modification site outside [-1, L], n_series = 0, 2^32 - 1 rows or more.  n = 0 stages an
 * empty library.  Effects on the handle as adh_stage_fragments; the host copy of the records is rebuilt by the host
 * team (adh_host_threads) from the same sums in the same order.  adh_calibration_time_ms covers the call's kernels.
 */
int adh_stage_candidate_library(adh_handle_t *handle, const adh_candidate_library_t *library,
                                const adh_loess_model_t *model, uint32_t *flat_frag_start_idx,
                                uint32_t *flat_frag_stop_idx, float *mz_library_out, double *mz_out);

/*
 * For tests and tools: the raw 32-byte records of the staged library, from HBM (host_mirror = 0) or from the
 * handle's host copy (host_mirror = 1).  Byte offsets: mz_library 0, mz 4, intensity 8 (float32); type 12,
 * loss_type 13, charge 14, number 15, position 16, cardinality 17 (uint8); 18 .. 31 zero.  n must be the staged
 * library's fragment count.
 */
int adh_staged_fragments_read(adh_handle_t *handle, int32_t host_mirror, void *records, int64_t n);

/* ------------------------------------------------------------------------------------------
 * Cross-run fragment quantity matrices of label-free quantification
 * (outputtransform/quantification/fragment_accumulator.py:51-101, quant_builder.py:52-182).
 * The frag rows of every run whose precursor is among the PSMs are appended in HBM, the union of
 * their ion keys over the runs is built with one stable radix sort, and each quantity column is
 * scattered into a zero-filled column-major n_keys x n_runs float32 matrix (NaN -> 0, fillna(0)).
 * The matrices stay in HBM for the filter calls that follow.
 * ------------------------------------------------------------------------------------------ */

#define ADH_QUANT_MAX_COLUMNS 16
typedef struct adh_quant adh_quant_t;

/* An empty accumulation of n_columns float32 quantity columns; psm_precursor_idx: the PSMs' precursors, sorted and
 * distinct (the frag rows of other precursors are dropped). */
int adh_quant_create(adh_handle_t *handle, int32_t n_columns, const uint32_t *psm_precursor_idx, int64_t n_psm,
                     adh_quant_t **quant);
int adh_quant_destroy(adh_quant_t *quant);
/* Append one run's frag table (n rows; columns[n_columns] float32 arrays): its rows of PSM precursors, with the ion
 * key precursor_idx + number << 32 + type << 40 + charge << 48 + loss_type << 56 in int64.  n_kept: rows kept. */
int adh_quant_add_run(adh_quant_t *quant, int64_t n, const uint32_t *precursor_idx, const uint8_t *number,
                      const uint8_t *type, const uint8_t *charge, const uint8_t *loss_type, const float *const *columns,
                      int64_t *n_kept);
/* The union of keys and the matrices.  One run: its kept rows in their order.  Two or more: the distinct keys in
 * ascending (signed) order.  If a run holds a key twice, *duplicate = 1, no matrix is built and the rows stay
 * readable through adh_quant_rows (the reference's merge makes a cartesian product of such keys). */
int adh_quant_build(adh_quant_t *quant, int64_t *n_keys, int32_t *duplicate);
/* ion[n_keys] (int64) and precursor_idx[n_keys] of the built union */
int adh_quant_keys(adh_quant_t *quant, int64_t *ion, uint32_t *precursor_idx);
/* quantity column `column` as n_keys x n_runs float32, column-major (run r at out + r * n_keys) */
int adh_quant_matrix(adh_quant_t *quant, int32_t column, float *out);
/* the appended rows in run order: ion, precursor_idx, run, columns[n_columns] (NaN as given) */
int adh_quant_rows(adh_quant_t *quant, int64_t *ion, uint32_t *precursor_idx, uint32_t *run, float *const *columns);
/* A fresh one-column object takes a quality matrix from the host instead (run_columns[n_runs] of n_keys floats). */
int adh_quant_set_matrix(adh_quant_t *quant, int64_t n_keys, int32_t n_runs, const float *const *run_columns);
/*
 * QuantBuilder.filter_frag_df (quant_builder.py:132-182) over matrix `column`: total[i] = the float32 mean of row i
 * over the runs, summed run after run as NumPy reduces the frame's F-ordered values; rank[i] =
 * rank(ascending=False, method="first") of total inside group[i] (codes 0 .. n_groups - 1; a negative code or a NaN
 * total gives NaN, as pandas does); mask[i] = rank <= top_n | total > threshold (compared in float64: pass the
 * threshold in the precision of the comparison it stands for).
 */
int adh_quant_filter(adh_quant_t *quant, int32_t column, const int32_t *group, int32_t n_groups, double top_n,
                     double threshold, float *total, double *rank, uint8_t *mask);
/* HIP-event times (ms) of the device work of adh_quant_build and of the last adh_quant_filter */
int adh_quant_time_ms(adh_quant_t *quant, double *build_ms, double *filter_ms);

/* ------------------------------------------------------------------------------------------
 * Protein inference: the greedy set cover of perform_grouping (outputtransform/grouping.py:8-194).
 * The host sends the distinct id strings of a precursor table as "patterns" weighted by their
 * number of precursors, and the deduplicated edge list (pattern, id code); id codes number the
 * ids in their order of first appearance, the two decoy classes with disjoint codes.  The device
 * labels the connected components of that graph and runs one cover per component: repeatedly the
 * id with the largest weight of uncovered patterns (the smallest code on a tie) becomes the master
 * of those patterns.  Strings stay on the host.
 * ------------------------------------------------------------------------------------------ */

typedef struct adh_pg adh_pg_t;

int adh_pg_create(adh_handle_t *handle, adh_pg_t **pg);
int adh_pg_destroy(adh_pg_t *pg);
/* One cover over n_edges distinct edges (edge_pattern[e] in [0, n_patterns), edge_id[e] in [0, n_ids)) and
 * weight[n_patterns] >= 0 (their sum below 2^31).  pattern_master[p]: the id that covers pattern p (-1: a pattern
 * no id with a positive weight holds); id_emptied_by[i]: the master whose claim took the last uncovered pattern of
 * id i (-1: none; masters themselves have -1).  Codes out of range, a negative weight or an edge count that the
 * sizes cannot hold fail with ADH_ERR_INVALID_ARGUMENT before anything is launched; the component labelling gives
 * up with ADH_ERR_HIP after a fixed number of rounds. */
int adh_pg_solve(adh_pg_t *pg, int32_t n_patterns, int32_t n_ids, int64_t n_edges, const int32_t *edge_pattern,
                 const int32_t *edge_id, const int32_t *weight, int32_t *pattern_master, int32_t *id_emptied_by);
/* The heuristic filter over the last cover: a string is allowed if an id that carries it (id_string[n_ids], codes in
 * [0, n_strings)) is a master; offsets[n_patterns + 1] and ids[*n_kept] (room for n_edges) give, per pattern, its ids
 * with an allowed string by ascending id_rank[n_ids]. */
int adh_pg_filter(adh_pg_t *pg, int32_t n_strings, const int32_t *id_string, const int32_t *id_rank, int32_t *offsets,
                  int32_t *ids, int64_t *n_kept);
/* components of the last cover, those of more than 64 ids among them, and the rounds the labelling took */
int adh_pg_stats(adh_pg_t *pg, int32_t *n_components, int32_t *n_large, int32_t *rounds);
/* HIP-event times (ms) of the last cover's component labelling (with the CSR build) and cover kernels, and of the
 * last filter */
int adh_pg_time_ms(adh_pg_t *pg, double *label_ms, double *cover_ms, double *filter_ms);

/* ------------------------------------------------------------------------------------------
 * Protein-group FDR: perform_protein_fdr (outputtransform/protein_fdr.py:15-112).  The host
 * factorises the strings: pg[i] is the rank of row i's protein group among the sorted distinct
 * groups (-1: the row has none), sequence[i] and run[i] are codes of any numbering.  The device
 * computes the features of every (pg, decoy) group, trains sklearn's MLPClassifier (float64,
 * 7 -> 100 ReLU -> 1 logistic, Adam) one epoch per call from parameters and row orders the host
 * draws, scores all groups, and hands a per-group value back to the rows.
 * ------------------------------------------------------------------------------------------ */

typedef struct adh_pfdr adh_pfdr_t;

int adh_pfdr_create(adh_handle_t *handle, adh_pfdr_t **pfdr);
int adh_pfdr_destroy(adh_pfdr_t *pfdr);
/* Groups the n_rows rows by (pg, decoy), ascending, and keeps per group in HBM: count, mean of proba, distinct
 * sequences, distinct precursor_idx, distinct runs, minimum and maximum of proba - the column order of the
 * reference's feature matrix.  proba is float32 (proba_is_f64 == 0) or float64; the mean is np.add.reduce over the
 * group's rows in table order (chunks of 8 192 elements added in order, pairwise inside a chunk) divided by the
 * count, both in proba's own type.  A pg code of 2^30 or more,
 * a decoy flag above 1 or a non-finite proba in a row that has a pg fail with ADH_ERR_INVALID_ARGUMENT /
 * ADH_ERR_UNSUPPORTED before anything is launched. */
int adh_pfdr_features(adh_pfdr_t *pfdr, int64_t n_rows, const int32_t *pg, const uint8_t *decoy,
                      const int64_t *precursor_idx, const int32_t *sequence, const int32_t *run, const void *proba,
                      int32_t proba_is_f64, int64_t *n_groups);
/* group_pg[n_groups], group_decoy[n_groups], features[n_groups * 7] (row-major) and, unless NULL,
 * row_group[n_rows] (-1: no group) of the last adh_pfdr_features */
int adh_pfdr_read_features(adh_pfdr_t *pfdr, int32_t *group_pg, uint8_t *group_decoy, double *features,
                           int32_t *row_group);
/* Stages x[n_train * 7] (row-major, scaled), the labels y[n_train] (0 / 1) and the 901 initial parameters
 * (W1 [7][100] row-major, b1 [100], W2 [100], b2); zeroes the Adam moments. */
int adh_pfdr_fit_begin(adh_pfdr_t *pfdr, int64_t n_train, const double *x, const uint8_t *y, const double *params);
/* One epoch in one launch on one workgroup: batches of min(200, n_train) rows in the order order[n_train] gives,
 * step k with Adam's step size step_size[k] (n_steps = the number of batches); *loss is the epoch's mean loss
 * (log-loss on clipped probabilities + 0.5 alpha |W|^2 / batch rows, alpha = 1e-4).  Every sum runs in a fixed order. */
int adh_pfdr_epoch(adh_pfdr_t *pfdr, const int32_t *order, int32_t n_steps, const double *step_size, double *loss);
/* proba[n]: the network's output for x[n * 7] under the current parameters; a row's value depends on that row only */
int adh_pfdr_predict(adh_pfdr_t *pfdr, int64_t n, const double *x, double *proba);
/* row_value[n_rows] = group_value[group of the row], NaN for a row of no group (the last adh_pfdr_features) */
int adh_pfdr_gather(adh_pfdr_t *pfdr, int64_t n_groups, const double *group_value, double *row_value);
/* HIP-event times (ms): the last adh_pfdr_features, all epochs since adh_pfdr_fit_begin, the last predict and gather */
int adh_pfdr_time_ms(adh_pfdr_t *pfdr, double *features_ms, double *epochs_ms, double *predict_ms, double *gather_ms);

/* ------------------------------------------------------------------------------------------
 * Transfer-learning library: TransferLearningAccumulator, normalize_rt_max / _delta_max and
 * ms2_quality_control (outputtransform/outputaccumulator.py:272-540).  An adh_tl_t keeps the
 * consensus in HBM: the sort keys and dense-row blocks of its precursors and n_matrices dense
 * float32 matrices of n_columns columns.  Strings and all other precursor columns stay with the
 * host, which truncates them with the kept-row index the device returns.
 * ------------------------------------------------------------------------------------------ */

#define ADH_TL_MAX_MATRICES 4
/* float32 values of LDS per wavefront in adh_tl_qc: a block with more cells of positive intensity takes the
 * workgroup path */
#define ADH_TL_QC_SLICE 512

typedef struct adh_tl adh_tl_t;

int adh_tl_create(adh_handle_t *handle, int32_t n_columns, int32_t n_matrices, adh_tl_t **tl);
int adh_tl_destroy(adh_tl_t *tl);
/* Stages one run from its flat fragment rows (needs n_matrices == 3: m/z, intensity, correlation): zero-filled
 * matrices of n_rows rows, flat row i written at (row[i], col[i]).  A cell written twice sets *duplicate and nothing
 * is staged.  A row or column outside the matrices fails before anything is launched. */
int adh_tl_scatter(adh_tl_t *tl, int64_t n_rows, int64_t n_flat, const int64_t *row, const int32_t *col, const float *mz,
                   const float *intensity, const float *correlation, int32_t *duplicate);
/* Appends a run of n_new precursors and n_new_rows dense rows (matrices[n_matrices], row-major host arrays; NULL: the
 * run adh_tl_scatter staged), orders all rows by (mod_seq_hash, proba, precursor_idx) ascending - stable, NaN proba
 * last; the hash is uint64 or, with hash_is_signed, int64 - keeps the first keep_top rows of every hash, drops the
 * dense rows of the others and renumbers the kept blocks in the order of their old start. */
int adh_tl_update(adh_tl_t *tl, int32_t keep_top, int64_t n_new, const void *mod_seq_hash, int32_t hash_is_signed,
                  const void *proba, int32_t proba_is_f64, const int64_t *precursor_idx, const int64_t *frag_start,
                  const int64_t *frag_stop, int64_t n_new_rows, const float *const *matrices, int64_t *n_kept,
                  int64_t *n_kept_rows);
/* kept[n_kept]: the rows of the last update as indices into "consensus before it, then the new run", in their new
 * order; frag_start / frag_stop[n_kept]: their renumbered blocks */
int adh_tl_read_kept(adh_tl_t *tl, int64_t *kept, int64_t *frag_start, int64_t *frag_stop);
/* matrix m of the consensus, [n_kept_rows * n_columns] row-major */
int adh_tl_read_matrix(adh_tl_t *tl, int32_t m, float *out);
/* HIP-event times (ms) of the last update's sort / keep mask and of its renumbering / row gathers, and of the last scatter */
int adh_tl_time_ms(adh_tl_t *tl, double *topk_ms, double *gather_ms, double *scatter_ms);
/* ms2_quality_control on host matrices [n_rows * n_columns]: per block the float32 median of the correlations at
 * cells with intensity > 0 (none: 0.0, and use_for_ms2 = empty_passes), use_for_ms2 = median > cutoff, every
 * intensity of the block multiplied by (correlation > median * ratio), in place.  *n_large: the blocks that took the
 * workgroup path. */
int adh_tl_qc(adh_handle_t *handle, int64_t n_precursors, const int64_t *frag_start, const int64_t *frag_stop,
              int64_t n_rows, int32_t n_columns, float *intensity, const float *correlation, float cutoff, float ratio,
              int32_t empty_passes, uint8_t *use_for_ms2, int64_t *n_large, double *kernel_ms);
/* rt_norm[n]: delta_max == 0: rt_observed / max(rt_observed), the maximum skipping NaN, in rt_observed's type;
 * else normalize_rt_delta_max with np.max (NaN propagates), every operation in the type NumPy's promotion of its
 * operands gives; the result is float32 only when all three columns are. */
int adh_tl_rt_norm(adh_handle_t *handle, int64_t n, int32_t delta_max, const void *rt_observed, int32_t observed_is_f64,
                   const void *rt_calibrated, int32_t calibrated_is_f64, const void *rt_library, int32_t library_is_f64,
                   void *rt_norm, double *kernel_ms);

/* ------------------------------------------------------------------------------------------
 * Match-between-runs library: MbrLibraryBuilder and IndexBuilder (libtransform/mbr.py).  An
 * adh_mbr_t keeps what one step leaves for the next in HBM: the two aggregate tables and the
 * elution groups that passed (adh_mbr_aggregate), the kept library rows and their dense rows
 * (adh_mbr_filter).  The host may change the library between adh_mbr_filter and adh_mbr_assign
 * (decoys).  Strings stay with the host: pg comes back as a row of the PSM table.
 * ------------------------------------------------------------------------------------------ */

typedef struct adh_mbr adh_mbr_t;

int adh_mbr_create(adh_handle_t *handle, adh_mbr_t **mbr);
int adh_mbr_destroy(adh_mbr_t *mbr);
/* The PSM table of n rows: rows with qval <= fdr (NaN fails) are aggregated by elution_group_idx (uint32 with
 * group_is_u32, else int64) and by mod_seq_charge_hash (uint64, or int64 with hash_is_signed): the distinct keys
 * ascending, the median of the non-NaN rt_observed (float32, or float64 with rt_is_f64; the mean of the two middle
 * values in float64, rounded to the column's type; NaN when all are NaN; -0.0 counts as +0.0) and the first row with
 * pg_notnull (-1: none).  The groups that passed are the distinct elution groups of the surviving rows, of those with
 * decoy == 0 unless keep_decoys.  *n_passed: surviving rows; *n_by_group / *n_by_hash: rows of the two tables. */
int adh_mbr_aggregate(adh_mbr_t *mbr, int64_t n, const double *qval, const uint8_t *decoy, const void *elution_group_idx,
                      int32_t group_is_u32, const void *mod_seq_charge_hash, int32_t hash_is_signed, const void *rt_observed,
                      int32_t rt_is_f64, const uint8_t *pg_notnull, double fdr, int32_t keep_decoys, int64_t *n_passed,
                      int64_t *n_by_group, int64_t *n_by_hash, int64_t *n_groups);
/* which 0: the table by elution group (keys as int64 values), 1: by hash (keys in the bits they came in), 2: the
 * groups that passed (keys only, as int64 values).  median in rt_observed's type. */
int adh_mbr_read_table(adh_mbr_t *mbr, int32_t which, void *keys, void *median, int64_t *first_row);
/* The library of n_lib precursors and n_rows dense rows: keeps the precursors whose elution group passed (library row
 * order), orders their blocks [frag_start, frag_stop) by ascending old start (stable), renumbers them by an exclusive
 * scan of their lengths and gathers the rows of matrices[n_matrices] (float32 [n_rows * n_columns] host arrays).
 * matrices NULL: only the source row of every kept dense row is computed (adh_mbr_read_filter). */
int adh_mbr_filter(adh_mbr_t *mbr, int64_t n_lib, const void *elution_group_idx, int32_t group_is_u32, const int64_t *frag_start,
                   const int64_t *frag_stop, int64_t n_rows, int32_t n_columns, int32_t n_matrices, const float *const *matrices,
                   int64_t *n_kept, int64_t *n_kept_rows);
/* kept[n_kept]: the kept library rows; frag_start / frag_stop[n_kept]: their renumbered blocks; source_row[n_kept_rows]
 * (may be NULL): the old dense row of every kept dense row */
int adh_mbr_read_filter(adh_mbr_t *mbr, int64_t *kept, int64_t *frag_start, int64_t *frag_stop, int64_t *source_row);
/* gathered matrix m, [n_kept_rows * n_columns] row-major */
int adh_mbr_read_matrix(adh_mbr_t *mbr, int32_t m, float *out);
/* Per precursor: rt[n] (the aggregate's rt type) and pg_row[n] (a PSM row, -1: null) from the hash table where the
 * hash was identified, from the elution-group table otherwise.  *n_missing: precursors whose elution group is in
 * neither (their rt is NaN, pg_row -1).  The hash has the aggregate's signedness. */
int adh_mbr_assign(adh_mbr_t *mbr, int64_t n, const void *elution_group_idx, int32_t group_is_u32, const void *mod_seq_charge_hash,
                   int32_t hash_is_signed, void *rt, int64_t *pg_row, int64_t *n_missing);
/* index[n_targets]: the position of every target key in lookup_keys, -1 when absent; keys in an order-preserving
 * uint64 form.  *duplicate: a lookup key occurs twice (index is then undefined). */
int adh_mbr_index(adh_mbr_t *mbr, int64_t n_targets, const uint64_t *target_keys, int64_t n_lookup, const uint64_t *lookup_keys,
                  int64_t *index, int32_t *duplicate);
/* The pg_notnull mask of a 1-d array of Python objects without a call per element (host only): out[i] = 0 where
 * items[i] is `none`, 1 where its type is `str_type`, 2 elsewhere; *n_other counts the 2s.  Only for interpreters whose
 * objects begin with the reference count and the type pointer (runtime.py probes that). */
int adh_mbr_notnull_objects(void *const *items, int64_t n, const void *none, const void *str_type, uint8_t *out,
                            int64_t *n_other);
/* HIP-event times (ms) of the last aggregate, filter (membership, renumbering), row gather and assign; bytes moved
 * host to device and device to host since adh_mbr_create */
int adh_mbr_stats(adh_mbr_t *mbr, double *aggregate_ms, double *filter_ms, double *gather_ms, double *assign_ms,
                  uint64_t *h2d_bytes, uint64_t *d2h_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ALPHADIA_HIP_H */
