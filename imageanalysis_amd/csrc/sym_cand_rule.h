// The candidate rule of the symmetric filter stage (match_knn2sym.hip, symcand_rows_kernel), in one
// place for the kernel and for the host test that walks it (tests/test_sym_cand_rule.py).
//
// A query row with bounds Lb <= (best squared distance) and (second squared distance) <= Ub is a
// CANDIDATE when the metric of the bounds can pass the threshold.  sym_cand_keep is that rule, in the
// arithmetic of the metric itself (two float32 roots, an f64 division, an f64 product).
// sym_cand_reject is a cheap test in front of it that only throws out rows the rule throws out:
//
//     reject  <=>  Ub > 0  and  Lb^2 >= K Ub,   K = thresh^2 (1 + 2^-20)
//
// The two float32 roundings, the division and the product put the computed metric at no less than
// (Lb / sqrt(Ub)) (1 - 2^-22); a rejected row has Lb / sqrt(Ub) >= thresh sqrt(1 + 2^-20), which is
// more than thresh / (1 - 2^-22): the rule does not keep it.  (Lb < 2^33: its square and K Ub are
// rounded once each, 2^-53 relative, far inside the margin.)  Everything the reject lets through goes
// to sym_cand_keep, so the candidate set is the rule's own -- not a superset of it.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SYM_CAND_FN __host__ __device__ inline
#else
#define SYM_CAND_FN inline
#endif

// K of sym_cand_reject for a threshold, computed ONCE on the host.  +inf (nothing is rejected early)
// for a threshold that is not finite and positive, and where thresh^2 leaves the normal range of a
// double: a K that underflowed to 0 would reject the rows with Lb == 0, which the rule keeps.
inline double sym_cand_K(double thresh)
{
    const double inf = HUGE_VAL;
    if (!(thresh > 0.0) || !(thresh < inf)) return inf;
    const double K = thresh * thresh * (1.0 + 0x1p-20);
    if (!(K >= 0x1p-1022) || !(K < inf)) return inf;
    return K;
}

SYM_CAND_FN bool sym_cand_reject(long long Lb, long long Ub, double K)
{
    const double l = (double)Lb;
    return Ub > 0 && l * l >= K * (double)Ub;
}

SYM_CAND_FN bool sym_cand_keep(long long Lb, long long Ub, double thresh)
{
    const float f0 = (float)sqrt((double)Lb);
    const float f1 = (float)sqrt((double)Ub);
    return f1 == 0.0f || (double)f0 * ((double)f0 / (double)f1) < thresh;
}
