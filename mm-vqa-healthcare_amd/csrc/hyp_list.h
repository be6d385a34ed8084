// The hypothesis list of one sample in the beam searches (csrc/beam.hip, csrc/trie_beam.hip): scores descending, a new entry goes
// AFTER entries of equal score (Python's stable sorted() on the appended list; a NaN score goes last), then the list is cut to nb.
#pragma once
#include "common.h"

namespace {

// Where `score` goes in hs[0..n), n <= nb, or -1 when it falls off a full list.  `last` = the index the current tail moves to (the
// old tail of a full list falls off): the caller moves entries last-1 .. p one up, writes entry p and calls hyp_count.
DEVINL int hyp_insert_pos(double score, int nb, int n, const double* hs, int& last) {
    int p = 0;
    while (p < n && !(hs[p] < score)) ++p;
    if (p >= nb) return -1;
    last = n < nb ? n : nb - 1;
    return p;
}
DEVINL int hyp_count(int n, int nb) { return n < nb ? n + 1 : n; }

}  // namespace
