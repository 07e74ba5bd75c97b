// The bit planes of an alignment's rows for the entries that scan them (sq_covar_dev.hip defines it; sq_covar.h has the
// layout): the checks the entries share -- a null d_rows, d_scratch or d_out, R < 1, L < 1, more than 2^31 tiles of 64 rows x
// 64 columns, scratch_bytes below sq_covariation_scratch(R, L): the error is set in `who`'s name and -1 returned with nothing
// enqueued --, then d_out's two words cleared and sq_covar_planes_kernel enqueued on st, the planes at the start of d_scratch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

int covar_planes(const char *who, const uint8_t *d_rows, int32_t R, int32_t L, void *d_scratch, size_t scratch_bytes, uint64_t *d_out,
                 hipStream_t st);

// The end of a pass 1 over the statistics of every pair of columns (sq_covar_stat_dev.hip defines it; sq_covar_stat.h has the
// order of the sums): sq_covar_stat_reduce_kernel and sq_covar_stat_total_kernel enqueued on st, d_mean[0 .. L] from the
// partial column sums.
int covar_stat_means(const double *partial, int32_t L, double *d_mean, hipStream_t st);

// The last launch of the statistics' nulls (sq_covar_stat_dev.hip defines it): sq_covar_stat_null_max_kernel enqueued on st,
// the K samples' maxima in d_key from integer keys to the bits of their doubles, in place.
int covar_stat_null_max(unsigned long long *d_key, int32_t K, hipStream_t st);

// Two launches of the weighted statistics, for their null (sq_covar_wstat_dev.hip defines them; sq_covar_wstat.h has the
// definitions): sq_covar_wstat_quantise_kernel enqueued on st -- d_q[rpad(R)] of the R weights, d_out[1] raised to 3 on a bad
// weight --, and sq_covar_wstat_sums_kernel, pass 1 of the planes of one alignment with the grid of sq_covariation_wstat_scan:
// its partial column sums, which covar_stat_means() then reduces.
int covar_wstat_quantise(const double *d_weights, int32_t R, uint32_t *d_q, uint64_t *d_out, hipStream_t st);
int covar_wstat_sums(const uint64_t *d_plane, const uint32_t *d_q, int32_t R, int32_t L, int32_t stat, double *d_partial, hipStream_t st);
