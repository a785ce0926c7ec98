// The last-block ticket: the coherent store / load pair and the ticket itself (device), and the
// ticket buffer that the fused split-K reduce (splitk_reduce.hip) and the optimizer's fused
// finalize (optimizer.hip) share (host).
#pragma once
#include "common.h"

namespace mnistx {

// Ticket ints of one (device, stream) buffer: one per partial-pass quad block of a fused reduce
// launch -- at most MAXRED descriptors of fewer than RED_MAX_QB quad blocks each -- then the
// optimizer's finalize ticket in a slot of its own.
constexpr int MAXRED = 8;         // descriptors of one reduce launch (RedTable)
constexpr int RED_MAX_QB = 512;   // a descriptor with this many quad blocks or more takes no partial pass
constexpr int OPT_TICKET_SLOT = MAXRED * RED_MAX_QB;
constexpr int TICKET_INTS = OPT_TICKET_SLOT + 64;
// The zeroed buffer of (current device, st), or nullptr: while st is being captured, or when the
// fused reduce is disabled and any_use is not set (splitk_reduce.hip).  Not part of the binding.
int* red_tickets(hipStream_t st, bool any_use = false);

namespace {

// agent-scope relaxed store / load: written through to / read from the coherence point (no
// L2-wide write-back or invalidate: the fences those need cost ~18 us in the LeNet-5 step and
// ~190 us in the reference CNN's when every block of a launch ran one)
DEV void st_coh(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEV float ld_coh(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The last-block ticket ("fence-free" hand-off; splitk_fused4_k, fused_opt_k):
//   every block: st_coh its partials -> take_ticket -> the block whose ticket is the last one
//   reads every block's partials with ld_coh and combines them.
// Memory-model argument.  In the HIP / C++ model the relaxed stores and the relaxed fetch_add
// carry no happens-before, so the language alone does not order them; the protocol rests on the
// gfx950 lowering of agent-scope relaxed atomics, which is the hand-off the microarchitecture
// guide (MI355X_MICROARCH.md, "Valid forms", first table row) measures as correct without an
// acquire: (1) st_coh is `global_store_* sc1` -- written through past the XCD's L2 to the
// coherence point; (2) `s_waitcnt vmcnt(0)` before the ticket: every such store of the issuing
// wave has completed (vmcnt counts stores) before the atomic is issued, and the storing wave is
// the ticket-taking wave (thread 0's wave after a __syncthreads in fused_opt_k; wave 0, which
// did all the stores, in splitk_fused4_k); (3) the winner's ld_coh is `global_load_* sc1`,
// served from the coherence point, never from a stale L1 / L2 line; (4) the winner's loads are
// control-dependent on the ticket's returned value.  The compiler must not move (1) below the
// ticket or (3) above it: the s_waitcnt builtin is not a compiler barrier, so both sides get a
// signal fence (compiler-only: no instruction).  tests/test_isa_ticket.py disassembles the
// built code object and fails if any of sc1 stores, sc1 loads or the vmcnt(0) before the ticket
// atomic goes missing (a compiler or flag change); release/acquire fences instead cost +20 us
// (LeNet-5) / +180 us (reference CNN) per step (profiles/r5/launch_fusion/README.md).
DEV int take_ticket(int* t) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_s_waitcnt(0);
  const int v = __hip_atomic_fetch_add(t, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  return v;
}

}  // namespace
}  // namespace mnistx
