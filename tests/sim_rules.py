"""The simulators' draws, restated (include/rmc.h RMC_SIM_*, DESIGN.md "Simulation
(config 4)"): the per-behaviour random stream, the choice of the initial state,
the packed kernel's reservoir pass (k_simulate), the wide kernels' uniform draw
with mode 0's exclude-and-redraw (uniform_draw) and TLC's start / prime-stride
draw over the model's action list (tlc_draw), and a predictor that walks N
behaviours with them.  Plain Python: no ctypes, no device.  Every draw is a
function of (seed, behaviour), so what a run replays and tallies is predicted
exactly; the predictor is given the enabled lanes of a state (the lane, whether
its successor is within the bounds, the successor) by its caller.

Lanes are those of the lane tables (raft_packed.h Lanes, raft_wide.h WLanes):
Restart S, Timeout S, RequestVote S*S, BecomeLeader S, ClientRequest S*VMAX,
AdvanceCommitIndex S, AppendEntries S*S, then Receive, DuplicateMessage and
DropMessage with one lane per bag slot."""
from dataclasses import dataclass, field

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
BEHAVIOUR = 0xD1B54A32D192ED03
PRIMES = (89, 97, 101, 103, 107, 109, 113, 127)
VMAX = 2        # ClientRequest lanes per server in every lane table
WIDE_SLOTS = 64  # bag slots of the wide layout (one lane each in families 7..9)
WITHIN_CAPACITY, TRUNCATE, TLC = 0, 1, 2


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Stream:
    """The splitmix64 stream of one behaviour."""

    def __init__(self, seed, b):
        self.rs = mix64(seed ^ ((b * BEHAVIOUR) & M64))
        self.drawn = 0

    def draw(self):
        self.rs = (self.rs + GOLDEN) & M64
        self.drawn += 1
        return mix64(self.rs)

    @classmethod
    def at(cls, rs, drawn=0):
        """A stream at a given position."""
        s = cls.__new__(cls)
        s.rs, s.drawn = rs, drawn
        return s

    def fork(self):
        return Stream.at(self.rs, self.drawn)


def init_index(stream, n_init):
    """One draw, also when there is one initial state."""
    return stream.draw() % n_init


# ---- the packed step (k_simulate) -----------------------------------------------
def packed_step(stream, lanes, mode):
    """lanes: (lane, in_bounds) of the enabled lanes in ascending lane order.
    Returns (pick, end): end None = the pick is taken, else "deadlocked" or
    "truncated"."""
    cnt, pick, pick_in = 0, -1, False
    for lane, inb in lanes:
        if mode == WITHIN_CAPACITY and not inb:
            continue  # before it consumes a draw
        cnt += 1
        if stream.draw() % cnt == 0:
            pick, pick_in = lane, inb
    if cnt == 0:
        return -1, "deadlocked"
    if not pick_in:
        return pick, "truncated"
    return pick, None


# ---- the wide uniform step (uniform_draw) ---------------------------------------
def uniform_draw(stream, enabled, excluded=()):
    """The k-th of the enabled lanes not excluded, in lane order, k = draw % their
    count; -1 (and no draw) when there is none."""
    cand = [l for l in sorted(enabled) if l not in excluded]
    if not cand:
        return -1
    return cand[stream.draw() % len(cand)]


def wide_uniform_step(stream, lanes, mode):
    """lanes as packed_step's.  Returns (pick, end, excluded lanes)."""
    inb = dict(lanes)
    excl = set()
    while True:
        pick = uniform_draw(stream, inb, excl)
        if pick < 0:
            return -1, ("truncated" if excl else "deadlocked"), excl
        if inb[pick]:
            return pick, None, excl
        if mode != WITHIN_CAPACITY:
            return pick, "truncated", excl
        excl.add(pick)  # mode 0: excluded for this step, and the draw repeated


# ---- the wide TLC step (tlc_draw) -----------------------------------------------
def wide_offsets(S):
    n = (S, S, S * S, S, S * VMAX, S, S * S, WIDE_SLOTS, WIDE_SLOTS, WIDE_SLOTS)
    off = [0]
    for k in n:
        off.append(off[-1] + k)
    return off


def tlc_actions(S, V):
    """Next's actions in order: ("lane", l) for every instance of Restart ..
    AppendEntries over the model's Server and Value sets, then ("family", lo, hi)
    for Receive, DuplicateMessage and DropMessage."""
    off = wide_offsets(S)
    acts = []
    for f in range(7):
        if f == 4:  # ClientRequest(i, v), v in the model's Value
            acts += [("lane", off[4] + i * VMAX + v) for i in range(S) for v in range(V)]
        else:
            acts += [("lane", l) for l in range(off[f], off[f + 1])]
    assert len(acts) == 2 * S + S * S + S + S * V + S + S * S
    acts += [("family", off[f], off[f + 1]) for f in (7, 8, 9)]
    return acts


def tlc_draw(stream, enabled, S, V):
    """enabled: the enabled lanes.  The lane drawn, -1 if none is enabled."""
    acts = tlc_actions(S, V)
    nact = len(acts)
    on = set(enabled)
    start = stream.draw() % nact
    stride = PRIMES[stream.draw() & 7]
    for i in range(nact):
        a = acts[(start + i * stride) % nact]
        if a[0] == "lane":
            if a[1] in on:
                return a[1]
            continue
        fam = [l for l in range(a[1], a[2]) if l in on]
        if fam:
            return fam[stream.draw() % len(fam)]
    return -1


def wide_tlc_step(stream, lanes, S, V):
    inb = dict(lanes)
    pick = tlc_draw(stream, inb, S, V)
    if pick < 0:
        return -1, "deadlocked"
    return pick, (None if inb[pick] else "truncated")


def plain(x):
    """A state (or a list of states) with its sets as sorted tuples: a form whose repr
    does not depend on the process's string hashing."""
    if isinstance(x, (set, frozenset)):
        return tuple(sorted((plain(y) for y in x), key=repr))
    if isinstance(x, (tuple, list)):
        return tuple(plain(y) for y in x)
    return x


# ---- the predictor --------------------------------------------------------------
@dataclass
class Walk:
    states: list
    end: str = "depth"  # "depth", "truncated", "deadlocked" or "violation"
    picks: list = field(default_factory=list)


@dataclass
class Prediction:
    walks: dict            # behaviour -> Walk
    steps: int = 0
    truncated: int = 0
    deadlocked: int = 0
    violation: tuple = None  # least (depth, index of the first violated invariant, behaviour)
    filtered_steps: int = 0  # mode 0: steps at which a lane was skipped / excluded
    diverted_steps: int = 0  # .. and the pick is not the one mode 1 would make there

    @property
    def tallies(self):
        return self.steps, self.truncated, self.deadlocked


def predict(layout, mode, inits, behaviours, depth, seed, expand, first_violated, S=3, V=2):
    """Walk the given behaviours (an iterable of behaviour numbers) to `depth`.
    inits: the initial states in the kernels' order.  expand(states) -> per state
    the list of (lane, in_bounds, successor or None) of its enabled lanes, in lane
    order; called once per step with the distinct current states.
    first_violated(state) -> the index of the first violated invariant, or None."""
    assert layout in ("packed", "wide") and (mode != TLC or layout == "wide")
    out = Prediction(walks={})
    live = {}
    for b in behaviours:
        st = Stream(seed, b)
        s = inits[init_index(st, len(inits))]
        w = Walk(states=[s])
        out.walks[b] = w
        v = first_violated(s)
        if v is not None:
            w.end = "violation"
            out.violation = min(out.violation or (1, v, b), (1, v, b))
        else:
            live[b] = st
    for dd in range(2, depth + 1):
        if not live:
            break
        cur = list(dict.fromkeys(out.walks[b].states[-1] for b in live))
        lanes_of = dict(zip(cur, expand(cur)))
        for b in list(live):
            st, w = live[b], out.walks[b]
            lanes = lanes_of[w.states[-1]]
            pairs = [(l, inb) for l, inb, _t in lanes]
            before = st.fork()
            if layout == "packed":
                pick, end = packed_step(st, pairs, mode)
                filtered = mode == WITHIN_CAPACITY and any(not inb for _l, inb in pairs)
                other = packed_step(before, pairs, TRUNCATE)[0] if filtered else pick
            elif mode == TLC:
                pick, end = wide_tlc_step(st, pairs, S, V)
                filtered, other = False, pick
            else:
                pick, end, excl = wide_uniform_step(st, pairs, mode)
                filtered = bool(excl)
                other = wide_uniform_step(before, pairs, TRUNCATE)[0] if filtered else pick
            out.filtered_steps += filtered
            out.diverted_steps += filtered and end is None and other != pick
            if end is not None:
                w.end = end
                if end == "truncated":
                    out.truncated += 1
                else:
                    out.deadlocked += 1
                del live[b]
                continue
            t = next(t for l, _inb, t in lanes if l == pick)
            w.states.append(t)
            w.picks.append(pick)
            out.steps += 1
            v = first_violated(t)
            if v is not None:
                w.end = "violation"
                out.violation = min(out.violation or (dd, v, b), (dd, v, b))
                del live[b]
    return out
