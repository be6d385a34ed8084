// The top-k scheme of the evaluation kernels (csrc/vqa_eval.hip, csrc/token_eval.hip): every value becomes the order key of
// csrc/order_key.h (eval_key: torch.argmax's rule); a thread keeps the kk greatest keys it has seen in its own column of an LDS
// table (cand[slot][thread]; 0 = empty, no key is 0).  The top-k of the workgroup's keys is a subset of the union of the threads'
// top-k, so rank j is "the greatest candidate below rank j - 1": kk passes over LDS, each a wave maximum and a four-way fold.  Keys of
// distinct columns are distinct integers: the result depends on no order.
#pragma once
#include "common.h"
#include "order_key.h"

namespace {

constexpr int KEEP_T = 256;      // threads of a workgroup that uses the scheme

// The kk greatest keys a thread has seen, in cand[slot * KEEP_T + tid]; mn / mnpos = the least of them and its slot.
struct Keep {
    uint64_t* c;
    int kk, mnpos;
    uint64_t mn;
    DEVINL void put(uint64_t key) {
        if (key <= mn) return;
        c[mnpos * KEEP_T] = key;
        mn = c[0];
        mnpos = 0;
        for (int s = 1; s < kk; ++s) {
            const uint64_t v = c[s * KEEP_T];
            if (v < mn) { mn = v; mnpos = s; }
        }
    }
};

// sel[j] = the key of rank j, j < kk, from cand[kk][KEEP_T] (every thread calls it; a thread reads its own column of cand only, so
// no barrier is needed between its puts and the call).  Ends with a barrier: sel is readable by every thread afterwards.
DEVINL void keep_select(const uint64_t* cand, int kk, uint64_t (*red)[KEEP_T / 64], uint64_t* sel, int tid) {
    uint64_t prev = 0;
    for (int j = 0; j < kk; ++j) {
        uint64_t best = 0;
        for (int s = 0; s < kk; ++s) {
            const uint64_t v = cand[s * KEEP_T + tid];
            if ((j == 0 || v < prev) && v > best) best = v;
        }
        best = wave_max_u64(best);
        if ((tid & 63) == 0) red[j & 1][tid >> 6] = best;
        __syncthreads();   // one barrier a pass: pass j + 2 reuses red[j & 1] only after every thread has passed the barrier of j + 1
        const uint64_t a = red[j & 1][0], b = red[j & 1][1], c = red[j & 1][2], d = red[j & 1][3];
        const uint64_t ab = a > b ? a : b, cd = c > d ? c : d;
        prev = ab > cd ? ab : cd;
        if (tid == 0) sel[j] = prev;
    }
    __syncthreads();
}

}  // namespace
