// The "ping-pong" LDS ring shared by the MFMA kernels that stage their operands with LDS-DMA (gemm_mfma.hip, xattn.hip, xflash.hip):
// the counted-wait rule, and the two-phase schedule with its ring-safety argument, which gemm_nt_pp_kernel, gemm_tn_pp_kernel and the
// NLOAD == 0 form of xg_kernel each run written out (why not as one template: the comment of gemm_nt_pp_kernel).
#pragma once
#include "mfma_tiles.h"

// ---- counted waits.  An LDS-DMA piece is a vector-memory load: vmcnt counts a wave's pieces and retires them IN ORDER, so
// "all but the youngest n chunks of this wave have landed" is s_waitcnt vmcnt(n * G), G = pieces per staging wave and chunk.  The
// operand of s_waitcnt is an immediate: a run-time n selects one of the instructions.
template <int N> DEVINL void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// MAX (<= 3) bounds the ladder: the most chunks the caller ever leaves in flight (a larger n waits as for MAX).
template <int G, int MAX = 3> DEVINL void wait_vm_chunks(int n) {
    static_assert(MAX >= 1 && MAX <= 3 && MAX * G <= 63, "vmcnt holds 6 bits");
    if (n > MAX) n = MAX;
    if (MAX >= 3 && n == 3) wait_vm<3 * G>();
    else if (MAX >= 2 && n == 2) wait_vm<2 * G>();
    else if (n == 1) wait_vm<G>();
    else wait_vm<0>();
}
// A ring of DEPTH + 1 slots keeps up to DEPTH chunks requested ahead of the one being consumed.  The prologue requests chunks
// 0 .. min(nc, DEPTH) - 1 and needs chunk 0: everything behind it may stay in flight.
template <int DEPTH> DEVINL int pp_inflight_prologue(int nc) { return (nc < DEPTH ? nc : DEPTH) - 1; }
// While chunk c is consumed (chunk c + DEPTH already requested, if it exists) chunk c + 1 must land: the chunks behind c + 1 -- nc - 2 - c
// of them exist, at most DEPTH - 1 are requested -- may stay in flight.  (Written as a clamp of that count: hipcc then folds the ladder
// of wait_vm_chunks into compares of nc - c itself; a select on "chunks after c >= 1" in front of the minimum cost the wgrad kernel
// 2 % at 3072 x 768 -- a min, a select and two more branches in front of every odd phase's barrier, profiles/r17_pp_ring_ab.log.)
template <int DEPTH> DEVINL int pp_inflight_next(int nc, int c) {
    const int behind = nc - 2 - c;
    return behind < 0 ? 0 : (behind < DEPTH - 1 ? behind : DEPTH - 1);
}

// ---- the two-phase schedule.  8 waves in two groups (one wave of each per SIMD) consume 32-deep reduction chunks from a ring of
// DEPTH + 1 slots; chunk c lives in slot c % (DEPTH + 1).  Each chunk is consumed in TWO phases -- the low / high half of the row
// blocks of the wave's sub-tile against the same column fragments, which stay in registers -- and a phase is
//     [LDS fragment reads + this wave's DMA issues]  s_barrier  [lgkmcnt(0); the MFMA cluster at raised priority]  s_barrier.
// The late group runs ONE barrier behind the early one, so on every SIMD one wave is in its MFMA cluster while the other
// fetches fragments and issues DMA: the MFMA pipe never waits for LDS.
//   phase 2c     reads B(c), A(c) low; issues B(c + DEPTH) into the slot of chunk c - 1
//   phase 2c + 1 reads A(c) high;      issues A(c + DEPTH); waits (counted) for chunk c + 1 BEFORE its first barrier
// (loads are issued in the order B(0) A(0) B(1) A(1) ..., G pieces per wave and chunk).
// Ring safety.  A wave's fragment reads of a phase are retired by the lgkmcnt(0) behind that phase's first barrier, i.e.
// before the wave arrives at the phase's second barrier.
//   RAW: every wave waits for its own pieces of chunk c + 1 before its first barrier of phase 2c + 1 and first reads the chunk
//        in phase 2c + 2, behind the second barrier of phase 2c + 1 -- a barrier every wave, of either group, passed post-wait.
//   WAR: B(c + DEPTH) overwrites B(c - 1), last read in phase 2c - 2: two phases (four barriers) before the issue, so that even
//        a late wave, one barrier behind the issuing early one, retired those reads at least two barriers ago.  A(c + DEPTH)
//        overwrites A(c - 1), last read (its high half) in phase 2c - 1: the same distance.
// After the loop the early group executes one more barrier: every wave has then executed 4 nc + 2 of them, all fragment reads are
// retired and no DMA is outstanding (the last odd phase waits for vmcnt(0)) -- the ring is free for the epilogue.
// The loader-wave kernels (xg_kernel with NLOAD == 4, xflash.hip) keep single-phase schedules of their own; their comments state
// only how those differ from the argument above.
