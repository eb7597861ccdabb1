// rmc_cover.h — action coverage (RMC_FLAG_COVERAGE, TLC -coverage): the rows of
// rmc_coverage and the rule that puts a lane of either layout into its row.
// Host and device: the coverage kernels (k_cover, k_wcover) and the host check
// (tests/native/cover_check.cpp) call the same functions.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "raft_packed.h"
#include "raft_wide.h"

namespace rmc {

// Rows in rmc.h's order (RMC_COV_ACTIONS): Init, the seven server families, the
// five disjuncts of Receive (raft.tla:393-403), DuplicateMessage, DropMessage.
constexpr int COV_ROWS = 15;
constexpr int COV_INIT = 0, COV_UPDATE_TERM = 8, COV_RECEIVE = 9, COV_DUPLICATE = 13, COV_DROP = 14;

// A lane of a family other than Receive (7).
RMC_HD int cover_family_row(int f) { return f < 7 ? 1 + f : f == 8 ? COV_DUPLICATE : COV_DROP; }
// A Receive lane, from the parent's message in its bag slot and currentTerm[mdest]
// (the rule of rmc-tlc's trace headers): UpdateTerm (raft.tla:373-379) when the
// message's term is newer, else the disjunct of its mtype (0..3 = RVQ, RVP, AEQ, AEP).
RMC_HD int cover_receive_row(u32 mterm, u32 current_term, u32 mtype) {
    return mterm > current_term ? COV_UPDATE_TERM : COV_RECEIVE + (int)mtype;
}

// Packed layout: the row of `lane` on parent (w, m).
template <int S, int K>
RMC_HD int cover_row(const Params& P, const u64 (&w)[S], const u32 (&m)[K], int lane) {
    const int f = lane_family(P, lane);
    if (f != 7) return cover_family_row(f);
    const u32 msg = selm<K>(m, lane - P.off[7]);
    return cover_receive_row(m_term(msg), w_ct(selw<S>(w, (int)m_dst(msg))), m_type(msg));
}

namespace wide {
// Wide layout: the row of `lane` on parent s (a Receive lane's slot is below s.nmsg).
template <class St>
RMC_HD int wcover_row(const WModel& M, const St& s, int lane) {
    const int f = M.L.family(lane);
    if (f != 7) return cover_family_row(f);
    const typename St::Msg& m = s.msg[lane - M.L.off[7]];
    return cover_receive_row(m.term, s.ct[m.dst], m.type);
}
}  // namespace wide

}  // namespace rmc
