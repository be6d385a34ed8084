// The (m, s) = (maximum, sum exp(x - m)) pair arithmetic of the log-sum-exp kernels (csrc/token_eval.hip, csrc/answer_trie.hip).
// A term is e(x, m) = x == m ? 1 : expf(x - m), which is expf(x - m) for finite values and keeps inf - inf out of the sum; two
// pairs merge as m' = fmaxf(m1, m2), s' = s1 e(m1, m') + s2 e(m2, m').  Every s is a sum of terms in [0, 1]: there is no inf * 0.
#pragma once
#include "common.h"
#include <math.h>

namespace {

DEVINL float exp_diff(float x, float m) { return x == m ? 1.0f : expf(x - m); }
DEVINL void ms_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = s * exp_diff(m, mn) + s2 * exp_diff(m2, mn);
    m = mn;
}

}  // namespace
