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
