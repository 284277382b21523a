// probe_score.hpp -- what the metrics of the probes (probe.hip) and their bootstrap (resample.hip) must agree on bit for bit: which cases
// are test cases and of which class, the prediction of a case and, for C > 2, its fp64 log-softmax scores.
#pragma once
#include "common.hpp"

namespace mdl {

// the class of a labeled case, -1 for an unlabeled one (a training case is struck out afterwards)
__device__ __forceinline__ int8_t probe_test_class(int label, int C) { return (label >= 0 && label < C) ? (int8_t)label : (int8_t)-1; }

// The prediction of one case from its decision values zs [cols].  cols == 1: z > 0.  Else the first maximum, and score[c * cstride] =
// log_softmax(zs)[c] in double.
__device__ __forceinline__ int probe_predict(const float* __restrict__ zs, int cols, double* __restrict__ score, int64_t cstride) {
    if (cols == 1) return zs[0] > 0.f ? 1 : 0;
    int pred = 0;
    float best = zs[0];
    for (int c = 1; c < cols; ++c)
        if (zs[c] > best) {                 // strictly greater: the lowest index wins a tie
            best = zs[c];
            pred = c;
        }
    double sum = 0.0;
    for (int c = 0; c < cols; ++c) sum += exp((double)zs[c] - (double)best);
    const double lse = (double)best + log(sum);
    for (int c = 0; c < cols; ++c) score[c * cstride] = (double)zs[c] - lse;
    return pred;
}

}  // namespace mdl
