// sq_scoring.h -- the arithmetic of ScoreStruct (SQRNdbnseq.py:861-899) and of the metrics against a known structure
// (:1252-1258) that the ranking tail (sq_tail_dev.hip) and the scoring of given structures (sq_score_dev.hip) share: Python's
// round(x, 3), the value of a base pair, TP / FP / FN / FS / PR / RC from the counts.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// ---- Python's round(x, 3) (SQRNdbnseq.py:891-893,1256-1258): the decimal nearest to the EXACT binary value, ties to
// even, then the double nearest to that decimal.  x = m 2^e exactly, so 1000 x = (1000 m) / 2^-e is an integer
// quotient and remainder in 64-bit arithmetic; k / 1000.0 is one correctly rounded division of exact integers, i.e. what
// strtod returns for the decimal's text.  Exact for |x| < 2^53 / 1000; beyond, *inexact is set (the host takes over).
__device__ __forceinline__ double sq_round3(double x, uint32_t *inexact)
{
    if (!(x == x) || fabs(x) == INFINITY) return x;
    const double ax = fabs(x);
    if (ax >= 4503599627370496.0) return x;                            // >= 2^52: an integer
    if (ax >= 9.0e12) { *inexact = 1; return x; }
    const unsigned long long bits = (unsigned long long)__double_as_longlong(ax);
    const int ex = (int)((bits >> 52) & 0x7FFull);
    unsigned long long m = bits & 0xFFFFFFFFFFFFFull;
    int e;
    if (ex == 0) e = -1074; else { m |= 1ull << 52; e = ex - 1075; }
    unsigned long long k;
    if (e >= 0) k = (m << e) * 1000ull;                                // (ax < 9e12: no overflow)
    else {
        const int E = -e;
        const unsigned long long p = m * 1000ull;                      // < 2^63
        if (E >= 64) k = 0ull;                                         // 1000 x < 1/2
        else {
            const unsigned long long q = p >> E, r = p & ((1ull << E) - 1ull), half = 1ull << (E - 1);
            k = q + ((r > half || (r == half && (q & 1ull))) ? 1ull : 0ull);
        }
    }
    const double res = (double)k / 1000.0;
    return x < 0 ? -res : res;
}

// ScoreStruct's value of a base pair (:863-868) from the letter codes of include/squarna_hip.h ('A' + code): GC 4.0,
// AU 1.5, GU -0.5, anything else 0.  Multiples of 1/2: a stem's sum is exact in any order.
__device__ __forceinline__ double sq_pair_value(int a, int b)
{
    const int A = 0, C = 2, G = 6, U = 20;
    if ((a == G && b == U) || (a == U && b == G)) return -0.5;
    if ((a == A && b == U) || (a == U && b == A)) return 1.5;
    if ((a == G && b == C) || (a == C && b == G)) return 4.0;
    return 0.0;
}

// TP / FP / FN / FS / PR / RC (:1252-1258) from the pairs both structures hold (tp), the predicted pairs (np) and the known
// ones (known_n); a ratio with an empty denominator is 1.
__device__ __forceinline__ void sq_prf_counts(int tp, int np, int known_n, double m[6], uint32_t *inexact)
{
    const int fp = np - tp, fn = known_n - tp;
    m[0] = tp; m[1] = fp; m[2] = fn;
    m[3] = (2 * tp + fp + fn) ? sq_round3(2.0 * tp / (double)(2 * tp + fp + fn), inexact) : 1.0;
    m[4] = (tp + fp) ? sq_round3((double)tp / (double)(tp + fp), inexact) : 1.0;
    m[5] = (tp + fn) ? sq_round3((double)tp / (double)(tp + fn), inexact) : 1.0;
}
