// k_propose.hip — raft_ticket_status: what became of each proposal, read on
// the canonical view (canon_view.hpp: every group word through CanonGroup,
// every entry through ring_form / canon_entry). Read-only for the state.
//   ticket_status_kernel<R>  one lane per ticket: the ticket as two 16-B
//        loads, per replica LastApplied, CommitIndex and the live window, and
//        the entry at the ticket's index only where it is live (Term and
//        Value); the 8-B result as one vector store at the ticket's position;
//        per state a ballot, and one atomicAdd per wave and state that occurs
//        (integer sums: order-independent, so deterministic).
// The rules are include/raftstep.h's ("client proposals");
// tests/propose_model.py restates them in numpy. Nothing adds to an int32
// index: top - K + 1 stays inside int32 (top >= 0, K >= 1).
// (propose_kernel, the way into the log, is a handler kernel: k_slow.inc.)
#include "canon_view.hpp"

namespace raftstep {

namespace {
// enum raft_ticket_state
enum : uint32_t { TK_COMMITTED = 0, TK_SUPERSEDED = 1, TK_PENDING = 2, TK_EVICTED = 3, TK_DROPPED = 4, TK_INVALID = 5,
                  TK_STATES = 6 };
}  // namespace

template <int R>
__global__ __launch_bounds__(256) void ticket_status_kernel(DevPlanes P, int raft, const uint4* tickets, uint32_t n,
                                                            uint2* out, unsigned long long* tot) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t state = TK_STATES;   // (a lane past the list: counted nowhere)
  if (i < n) {
    const uint4 a = tickets[size_t(i) * 2u], b = tickets[size_t(i) * 2u + 1u];
    const int64_t value = int64_t(uint64_t(a.z) | (uint64_t(a.w) << 32));
    const uint32_t g = b.x;
    const int index = int(b.y), term = int(b.z);
    const CanonGroup<R> c(P, g);
    uint32_t replica = 0xFFu, holders = 0, committed = 0;
    if ((b.w & 0xFFu) != 1u || index <= 0) {   // not RAFT_PROPOSE_ACCEPTED: nothing to look for
      state = TK_INVALID;
    } else {
      const RingForm rf = ring_form(P, g);
      const int K = int(P.K);
      int wit = -1, holder = -1;          // lowest decided replica with a live entry, lowest holder
      bool wit_same = false, dec_gone = false, gone = false;
#pragma unroll 1
      for (int r = 0; r < R; ++r) {
        const int l = c.last(P, r);
        if (index > l) continue;          // absent
        const int top = max(c.hwm(P, r, raft, l), l);
        const int lo = max(1, top - K + 1);
        const bool decided = index <= min(c.commit(P, r), l);
        if (index < lo) {                 // gone: the entry has left the ring
          gone = true;
          dec_gone |= decided;
          continue;
        }
        const Entry en = canon_entry<R>(P, rf, g, uint32_t(r), index, EW_TERM | EW_VALUE);
        const bool same = en.term == term && en.value == value;
        if (same) {
          holders |= 1u << r;
          if (decided) committed |= 1u << r;
          if (holder < 0) holder = r;
        }
        if (decided && wit < 0) {
          wit = r;
          wit_same = same;
        }
      }
      if (wit >= 0) {
        state = wit_same ? TK_COMMITTED : TK_SUPERSEDED;
        replica = uint32_t(wit);
      } else if (dec_gone) {
        state = TK_EVICTED;
      } else if (holder >= 0) {
        state = TK_PENDING;
        replica = uint32_t(holder);
      } else {
        state = gone ? TK_EVICTED : TK_DROPPED;
      }
    }
    // raft_ticket_result: state, replica, fault, holders | committed, reserved[3]
    if (out) out[i] = uint2{state | (replica << 8) | (uint32_t(c.fault) << 16) | (holders << 24), committed};
  }
  if (tot) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = 0; k < TK_STATES; ++k) {
      const unsigned long long m = __ballot(state == k);
      if (lane == 0 && m) atomicAdd(&tot[k], (unsigned long long)__popcll(m));
    }
  }
}

hipError_t launch_ticket_status(int R, const DevPlanes& P, int raft, const void* tickets, uint32_t n, void* out,
                                unsigned long long* tot, hipStream_t s) {
  RAFT_DISPATCH_R(R, hipLaunchKernelGGL(ticket_status_kernel<RR>, grid_for(n), dim3(256), 0, s, P, raft,
                                        static_cast<const uint4*>(tickets), n, static_cast<uint2*>(out), tot));
  return hipGetLastError();
}

}  // namespace raftstep
