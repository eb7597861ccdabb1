"""The oracle of RMC_FLAG_CONTINUE (TLC -continue): a level-synchronous BFS over
oracle/raft_spec.py that does not stop at a violation (R.bfs does), counting per
invariant the stored states that violate it.  Shared by the generator of
tests/golden/continue_cases.json (tests/golden/make_continue_golden.py) and by
tests/test_continue.py, which recomputes the smallest case live.

Per stored state and mask: `first` = the lowest bit of the mask whose predicate
fails (the notion of rmc_result.violated_inv), `each` = every bit of the mask
whose predicate fails on its own; depth[r] = the level of the shallowest state
that fails r."""
from oracle import raft_spec as R

BITS = sorted(R.INV_BITS)  # 1, 2, 4, ..., 512: row r is bit 1 << r
ALL = sum(BITS)

# name: ((S, V, MaxTerm, MaxLog, MaxMsgs, MaxDup), bug, symmetry, max_depth (0: to fixpoint), mask)
CASES = {
    "bug_small_d12": ((3, 2, 2, 1, 1, 1), 1, 0, 12, ALL),
    "bug_small_sym_d12": ((3, 2, 2, 1, 1, 1), 1, 1, 12, ALL),
    "bug_s2_msgs2_full": ((2, 1, 2, 1, 2, 1), 1, 0, 0, ALL),
    "bug_msgs5_d9": ((3, 2, 2, 1, 5, 1), 1, 0, 9, ALL),
    "bug_s5_d8": ((5, 2, 2, 1, 2, 1), 1, 0, 8, ALL),
    "small_d15": ((3, 2, 2, 1, 1, 1), 0, 0, 15, ALL),
    "tiny2_full": ((2, 1, 2, 1, 2, 1), 0, 0, 0, ALL),
    # specs/MCraftMessages.cfg (rmc-tlc -continue): the `small` bounds to fixpoint, TypeOK and MessagesInv
    "cli_messages_small": ((3, 2, 2, 1, 1, 1), 0, 0, 0, 1 | 8),
}
SMALLEST = "tiny2_full"


def model_of(bounds, bug):
    S, V, mt, ml, mm, md = bounds
    return R.Model(n_servers=S, n_values=V, max_term=mt, max_log=ml, max_msgs=mm, max_dup=md, bug_quorum=bool(bug))


def continue_bfs(bounds, bug=0, symmetry=0, max_depth=0, mask=ALL):
    """The record of one case: what a run with the flag must report."""
    model = model_of(bounds, bug)
    key = (lambda t: R.canonical(model, t)) if symmetry else (lambda t: t)
    checks = [(r, R.INVARIANTS[R.INV_BITS[b]]) for r, b in enumerate(BITS) if mask & b]
    first, each, inv_depth = [0] * len(BITS), [0] * len(BITS), [0] * len(BITS)
    states = 0

    def classify(level, depth):
        nonlocal states
        for s in level:
            failed = [r for r, check in checks if not check(model, s)]
            if not failed:
                continue
            states += 1
            first[failed[0]] += 1
            for r in failed:
                each[r] += 1
                inv_depth[r] = inv_depth[r] or depth
    s0 = R.init_state(model)
    seen = {key(s0)}
    frontier = [s0]
    generated, depth, level_new = 1, 1, [1]
    classify(frontier, 1)  # the seed's states
    while frontier and (not max_depth or depth < max_depth):
        nxt = []
        for s in frontier:
            for _f, _p, t in R.successors(model, s):
                generated += 1
                if not R.in_constraint(model, t):
                    continue
                k = key(t)
                if k in seen:
                    continue
                seen.add(k)
                nxt.append(t)
        if nxt:
            depth += 1
            level_new.append(len(nxt))
            classify(nxt, depth)  # the last level too, though it is never expanded
        frontier = nxt
    return dict(params=dict(n_servers=bounds[0], n_values=bounds[1], max_term=bounds[2], max_log_len=bounds[3],
                            max_msgs=bounds[4], max_dup=bounds[5], bug_quorum=bug, symmetry=symmetry,
                            max_depth=max_depth, invariants=mask),
                distinct=len(seen), generated=generated, depth=depth, left_on_queue=len(frontier),
                level_new=level_new, states=states, first=first, each=each, inv_depth=inv_depth)


def run_case(name):
    bounds, bug, sym, max_depth, mask = CASES[name]
    return continue_bfs(bounds, bug, sym, max_depth, mask)
