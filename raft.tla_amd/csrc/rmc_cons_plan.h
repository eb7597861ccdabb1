// rmc_cons_plan.h — the index arithmetic of the constraint pass's in-place compaction
// (rmc_dev_cons.h; DESIGN.md "Model-defined constraints").  The kernels and the host test
// (tests/native/cons_check.cpp) run the same functions.
//
// A launch added the states at positions [0, n) of its new range; keep[p] says whether
// position p stays.  With `kept` of them staying, r = n - kept leave.  The head is
// [0, kept), the tail [kept, n).  The head has as many holes (positions that leave) as
// the tail has movers (positions that stay): m <= min(kept, r).  Every mover goes into a
// hole, paired by rank, so sources (tail) and destinations (head) are disjoint: the move
// is safe in place and in parallel, at most r states move, and afterwards [0, kept) holds
// exactly the kept states.  Ranks come from the kept counts of tiles of kConsTile
// positions (one block's worth), their exclusive scan, and a position's rank inside its
// tile:
//   kept_rank(p) = kept positions before p = tile_prefix[p / kConsTile] + in_tile_rank(p);
//   a hole's rank   = holes before it = p - kept_rank(p)        (ascending, 0 .. m-1);
//   a mover's rank  = kept positions after it = kept - 1 - kept_rank(p)   (0 .. m-1):
//     the movers are the last m kept positions, so no count of the tail's start is needed.
// Holes write their position into dst[hole rank]; the mover of rank j then goes to dst[j].
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "raft_packed.h"  // RMC_HD

namespace rmc {
namespace cons {

constexpr uint64_t kConsTile = 256;

RMC_HD uint64_t tiles(uint64_t n) { return (n + kConsTile - 1) / kConsTile; }
RMC_HD uint64_t kept_rank(uint64_t tile_prefix, uint32_t in_tile_rank) { return tile_prefix + in_tile_rank; }
RMC_HD bool is_hole(uint64_t p, uint64_t kept, bool keep) { return p < kept && !keep; }
RMC_HD bool is_mover(uint64_t p, uint64_t kept, bool keep) { return p >= kept && keep; }
RMC_HD uint64_t hole_rank(uint64_t p, uint64_t kept_rank_of_p) { return p - kept_rank_of_p; }
RMC_HD uint64_t mover_rank(uint64_t kept, uint64_t kept_rank_of_p) { return kept - 1 - kept_rank_of_p; }
// the kept positions before lane `lane` of a wave whose lanes' keep bits are `ballot`
RMC_HD uint32_t lane_rank(uint64_t ballot, int lane) {
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}

}  // namespace cons
}  // namespace rmc
