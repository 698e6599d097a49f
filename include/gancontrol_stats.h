/*
 * gancontrol_stats.h -- C ABI of the streaming feature statistics (csrc/feature_stats.hip): raw float64 moments of float32 feature rows,
 * accumulated batch by batch on the device, and the mean / covariance they finish into (fid_utils/feature_stats.py: FID without a host
 * copy of the features).
 *
 * Conventions of gancontrol_hip.h: raw device pointers, explicit extents, the HIP stream LAST (as void*), asynchronous launches, no
 * allocation, no global state; 0 on success, a negative GC_ERR_* code otherwise, with the text behind the main header's error query.
 * The library's version and struct checks are the main header's; this header declares no struct.
 *
 * The accumulator of F features is the pair
 *     s1 [F]     float64:  s1[i]    = sum_k x[k][i]
 *     s2 [F, F]  float64:  s2[i][j] = sum_k x[k][i] * x[k][j]     for j >= i
 * over every row k appended so far.  ONLY the upper triangle (j >= i) of s2 is defined: the accumulate entry may write any value into the
 * other elements of the GC_STATS_TILE x GC_STATS_TILE tiles on the diagonal and never touches the tiles below it; merge and finish read
 * the upper triangle only.  A fresh accumulator is all zeros.
 *
 * Arithmetic and error bound.  Every product is formed in float64 from two widened floats and is therefore exact (24 + 24 <= 53 bits).
 * The sums run on v_mfma_f64_16x16x4_f64, rows in ascending order, the running total carried from call to call; whatever the order of
 * the additions inside one instruction, a sum of n terms in ANY order satisfies
 *     |s2[i][j] - exact| <= gamma_n * sum_k |x[k][i] x[k][j]|,     |s1[i] - exact| <= gamma_n * sum_k |x[k][i]|,
 *     gamma_n = n u / (1 - n u),  u = 2^-53,  n = all rows appended so far.
 * Finish forms (s2[i][j] - s1[i] s1[j] / n) / (n - 1): one multiplication, one division, one subtraction and one more division, four
 * roundings on top of the errors of its operands, so with P = sum_k |x_ki x_kj| and A_i = sum_k |x_ki|
 *     |cov[i][j] - exact| <= (2 gamma_n + 8 u) (P + A_i A_j / n) / (n - 1),      |mean[i] - exact| <= (gamma_n + u) A_i / n.
 * No atomics, no flags, no workspace: one workgroup owns one tile of s2 and adds to it alone, so the same sequence of calls gives the
 * same bits.
 */
#ifndef GANCONTROL_STATS_H
#define GANCONTROL_STATS_H

#include "gancontrol_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GC_STATS_MAX_FEATURES 4096 /* 1 <= F <= this; beyond: GC_ERR_UNSUPPORTED */
#define GC_STATS_TILE 64           /* edge of the s2 tile one workgroup owns */

/* s1 += column sums of x, upper s2 += x^T x, for x [n, F] float32 with rows `stride` >= F elements apart (unit element stride; a
 * strided row view or a pitched buffer is read in place; any 4-byte alignment).  Rows past n - 1 and columns past F - 1 are zeros inside
 * the kernel: no byte outside the n rows of F elements is read.  One launch; grid = the F / 64 (rounded up) tiles on or above the diagonal.
 * GC_ERR_BAD_ARG: null pointer, n < 1, F < 1, stride < F.  GC_ERR_UNSUPPORTED: F > GC_STATS_MAX_FEATURES, or n * stride beyond int64. */
int gc_feature_moments_accumulate_f32(const float* x, int64_t stride, int n, int features, double* s1, double* s2, gc_stream_t stream);

/* mean[i] = s1[i] / n and the FULL symmetric cov[i][j] = (s2[a][c] - s1[a] s1[c] / n) / (n - 1) with (a, c) = (min, max)(i, j): both
 * triangles are written from the same operands in the same order, so cov is exactly symmetric.  n: the rows the accumulator holds, >= 2
 * (the divisor is numpy.cov's).  mean [F] and cov [F, F] are dense float64 and must not overlap the accumulator.
 * GC_ERR_BAD_ARG: null pointer, n < 2, F < 1.  GC_ERR_UNSUPPORTED: F > GC_STATS_MAX_FEATURES. */
int gc_feature_moments_finish_f64(const double* s1, const double* s2, int64_t n, int features, double* mean, double* cov, gc_stream_t stream);

/* s1a += s1b and s2a[i][j] += s2b[i][j] for j >= i: the accumulator of the union of two samples (raw moments are additive).  The other
 * elements of s2a keep their bits.  GC_ERR_BAD_ARG: null pointer, F < 1.  GC_ERR_UNSUPPORTED: F > GC_STATS_MAX_FEATURES. */
int gc_feature_moments_merge_f64(double* s1a, double* s2a, const double* s1b, const double* s2b, int features, gc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GANCONTROL_STATS_H */
