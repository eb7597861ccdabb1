// Host check of the sharded BFS's round arithmetic (rmc_dist_plan.h) and of the
// set-epoch decision (rmc_plan.h next_set_epoch).
//  1. W ranks are played on the host, W in {1, 2, 3, 8, 64}: key counts per
//     (source, destination) drawn from a fixed seed — zeros, full outboxes and a
//     rank that sends nothing among them — are laid out as k_pack_counts and the
//     count all-to-all lay out every rank's row, every rank decodes its row, and
//     the ranks' plans of the three all-to-alls must agree with one another and
//     stay inside their buffers.
//  2. round sizing over a grid, against the expressions of the loop before they
//     became functions (old_*: copied from it, the reference).
//  3. the set-epoch decision against the `if` it replaced.
// Build: g++ -O2 -std=c++17 -I raft.tla_amd/csrc dist_plan_check.cpp
// Run:   ./a.out   (prints "ok ..." or the first failure)
#include <cstdio>
#include <vector>

#include "rmc_dist_plan.h"
#include "rmc_plan.h"

using namespace rmc_host;
typedef uint64_t u64;
typedef unsigned long long ull;

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            printf("FAIL %s: ", #cond);       \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            return 1;                         \
        }                                     \
    } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() {  // splitmix64
    u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr u64 RWD = 17;   // kRowWords of the library: 2 + sizeof(Counters) / 8
constexpr u64 KEYB = 12;  // key record
constexpr u64 RB = 56;    // state record of S = 3, K = 4: (10 + 4) * 4

// One round of a world of W: returns 0 if every rank's plan agrees.
static int play_round(int W, u64 kcap, u64 ovf_cap, int trial) {
    const size_t w = (size_t)W;
    const CountRow L{RWD, (u64)W};
    CHECK(L.len() == 2 * RWD * (u64)W + 1 && L.novf() == RWD * (u64)W && L.recv(0) == L.novf() + 1 &&
              L.sent(W - 1) + RWD == L.novf() && L.recv(W - 1) + RWD == L.len(),
          "row layout, W %d", W);
    // keys a sends b; rank `empty` sends nothing; trial 0: nobody sends
    const int empty = W / 2, park_rank = trial % 5 == 3 ? (int)(rnd() % (u64)W) : -1;
    std::vector<u64> n(w * w, 0), acc(w * w, 0), flags(w), novf(w), known(w);
    for (int a = 0; a < W; ++a)
        for (int b = 0; b < W; ++b) {
            if (a == b || a == empty || trial == 0) continue;
            const u64 pick = rnd() % 4;
            n[a * w + b] = pick == 0 ? 0 : pick == 1 ? kcap : rnd() % (kcap + 1);
            acc[a * w + b] = n[a * w + b] ? rnd() % (n[a * w + b] + 1) : 0;  // those b accepts as new
        }
    for (int a = 0; a < W; ++a) {
        bool sends = false;
        for (int b = 0; b < W; ++b) sends |= n[a * w + b] != 0;
        novf[(size_t)a] = rnd() % 3 == 0 ? ovf_cap + 1 + rnd() % 100 : rnd() % (ovf_cap + 1);
        known[(size_t)a] = rnd() % 2 ? rnd() % (ovf_cap + 50) : 0;
        flags[(size_t)a] = (rnd() % 2 ? kFlagMore : 0) | (a == park_rank ? kFlagParkFull : 0) | (sends ? kFlagSends : 0);
    }
    // every rank's row: what it packed for each peer, then what each peer packed for it
    std::vector<std::vector<u64>> row(w, std::vector<u64>(L.len(), 0));
    for (int a = 0; a < W; ++a) {
        for (int p = 0; p < W; ++p) {
            u64* s = &row[(size_t)a][L.sent(p)];
            s[kRowKeys] = n[a * w + p];
            s[kRowFlags] = flags[(size_t)a];
            for (u64 i = kRowCounters; i < RWD; ++i) s[i] = 1000 * (u64)a + i;
        }
        row[(size_t)a][L.novf()] = novf[(size_t)a];
    }
    for (int a = 0; a < W; ++a)
        for (int p = 0; p < W; ++p)
            for (u64 i = 0; i < RWD; ++i) row[(size_t)a][L.recv(p) + i] = row[(size_t)p][L.sent(a) + i];

    std::vector<RoundPlan> rp;
    bool any_more = false, any_sends = false;
    for (int a = 0; a < W; ++a) {
        rp.push_back(decode_round(row[(size_t)a].data(), L, kcap, ovf_cap, known[(size_t)a], KEYB));
        any_more |= (flags[(size_t)a] & kFlagMore) != 0;
        any_sends |= (flags[(size_t)a] & kFlagSends) != 0;
    }
    for (int a = 0; a < W; ++a) {
        const RoundPlan& r = rp[(size_t)a];
        CHECK(r.park_full == park_rank, "W %d rank %d sees parking-full rank %d, it is %d", W, a, r.park_full, park_rank);
        CHECK(r.global_more == any_more && r.global_sends == any_sends, "W %d rank %d: global flags", W, a);
        CHECK(r.novf == std::min(novf[(size_t)a], ovf_cap), "W %d rank %d: novf %llu not clamped to %llu", W, a,
              (ull)r.novf, (ull)ovf_cap);
        CHECK(r.newly_parked <= r.novf && r.newly_parked == (r.novf > known[(size_t)a] ? r.novf - known[(size_t)a] : 0),
              "W %d rank %d: newly_parked %llu (novf %llu, known %llu)", W, a, (ull)r.newly_parked, (ull)r.novf,
              (ull)known[(size_t)a]);
        u64 in = 0, out = 0, mx = 0;
        for (int b = 0; b < W; ++b) {
            const RoundPlan& q = rp[(size_t)b];
            // what a plans to send b is what b plans to receive from a
            CHECK(r.keys.scnt[b] == q.keys.rcnt[a] && r.keys.scnt[b] == n[a * w + b] * KEYB,
                  "W %d keys %d -> %d: %llu sent, %llu expected", W, a, b, (ull)r.keys.scnt[b], (ull)q.keys.rcnt[a]);
            CHECK(r.replies.scnt[b] == q.replies.rcnt[a] && r.replies.scnt[b] == n[b * w + a],
                  "W %d replies %d -> %d: %llu sent, %llu expected", W, a, b, (ull)r.replies.scnt[b],
                  (ull)q.replies.rcnt[a]);
            // receive offsets: the prefix sums in rank order; send blocks: [W][kcap]
            CHECK(r.keys.roff[b] == in * KEYB && r.replies.soff[b] == in, "W %d rank %d: receive offset of %d", W, a, b);
            CHECK(r.keys.soff[b] == (u64)b * kcap * KEYB && r.replies.roff[b] == (u64)b * kcap,
                  "W %d rank %d: outbox offset of %d", W, a, b);
            // every block inside its buffer of W * kcap records
            const u64 room = (u64)W * kcap;
            CHECK(r.keys.soff[b] + r.keys.scnt[b] <= room * KEYB && r.keys.roff[b] + r.keys.rcnt[b] <= room * KEYB &&
                      r.replies.soff[b] + r.replies.scnt[b] <= room && r.replies.roff[b] + r.replies.rcnt[b] <= room,
                  "W %d rank %d: a block of peer %d leaves its buffer", W, a, b);
            // ... and inside its own [kcap] slice where the buffer is sliced per peer
            CHECK(r.keys.scnt[b] <= kcap * KEYB && r.replies.rcnt[b] <= kcap, "W %d rank %d: slice of %d", W, a, b);
            in += n[b * w + a];
            out += n[a * w + b];
            mx = std::max(mx, n[a * w + b]);
        }
        CHECK(r.keys.scnt[a] == 0 && r.keys.rcnt[a] == 0, "W %d rank %d sends itself keys", W, a);
        CHECK(r.tot_in == in && r.keys_sent == out && r.mx == mx, "W %d rank %d: tot_in / keys_sent / mx", W, a);
    }
    // phase 2, plain and verifying.  sa of rank a: [p] the states for p — its
    // own entry holds a count too (k_materialize_remote never adds to it; the
    // plan must not ship it) — and [W + p] the states from p
    for (int verify = 0; verify < 2; ++verify) {
        std::vector<StatePlan> sp;
        for (int a = 0; a < W; ++a) {
            std::vector<u64> sa(2 * w);
            for (int p = 0; p < W; ++p) {
                sa[(size_t)p] = p == a ? 7 : verify ? n[a * w + p] : acc[a * w + p];
                sa[w + (size_t)p] = p == a ? 5 : acc[p * w + a];  // (verification reads the row instead)
            }
            sp.push_back(state_blocks(sa.data(), row[(size_t)a].data(), L, a, kcap, RB, verify != 0));
        }
        for (int a = 0; a < W; ++a) {
            const StatePlan& s = sp[(size_t)a];
            CHECK(!s.over, "W %d rank %d: over", W, a);
            CHECK(s.states.scnt[a] == 0 && s.states.rcnt[a] == 0, "W %d rank %d sends itself states", W, a);
            u64 in = 0, out = 0, keys_in = 0;
            for (int b = 0; b < W; ++b) {
                CHECK(s.states.scnt[b] == sp[(size_t)b].states.rcnt[a], "W %d verify %d states %d -> %d: %llu sent, %llu expected",
                      W, verify, a, b, (ull)s.states.scnt[b], (ull)sp[(size_t)b].states.rcnt[a]);
                CHECK(s.states.roff[b] == in * RB && s.states.soff[b] == (u64)b * kcap * RB, "W %d rank %d: state offsets of %d",
                      W, a, b);
                const u64 room = (u64)W * kcap * RB;
                CHECK(s.states.soff[b] + s.states.scnt[b] <= room && s.states.roff[b] + s.states.rcnt[b] <= room &&
                          s.states.scnt[b] <= kcap * RB,
                      "W %d rank %d: a state block of peer %d leaves its buffer", W, a, b);
                in += s.states.rcnt[b] / RB;
                out += s.states.scnt[b] / RB;
                keys_in += n[b * w + a];
            }
            CHECK(s.tot_st == in && s.states_sent == out, "W %d rank %d: tot_st / states_sent", W, a);
            if (verify) CHECK(s.tot_st == keys_in && s.tot_st == rp[(size_t)a].tot_in, "W %d rank %d: verification receives every key's state", W, a);
        }
    }
    if (W > 1) {  // more accepted states for a peer than keys fit: reported, for a peer only
        std::vector<u64> sa(2 * w, 0);
        sa[0] = kcap + 1;
        CHECK(state_blocks(sa.data(), row[1].data(), L, 1, kcap, RB, false).over, "W %d: over not seen", W);
        CHECK(!state_blocks(sa.data(), row[0].data(), L, 0, kcap, RB, false).over, "W %d: over for the rank itself", W);
    }
    return 0;
}

// ---- round sizing: the loop's expressions before they became functions
constexpr int kMaxLaunchLog2 = 25;
struct OldD {
    int split;
    double fill;
};
static u64 old_split_cap(u64 frontier, const OldD& D) {
    const u64 split_cap = frontier >= (1ull << 21) ? (frontier + D.split - 1) / (u64)D.split : frontier;
    return split_cap;
}
static u64 old_round(u64 hi, u64 cursor, u64 kcap, double rho, u64 split_cap, const OldD& D, u64* cap_out) {
    const u64 target = (u64)(D.fill * (double)kcap / std::max(rho, 0.02));
    const u64 cap = std::max<u64>(1, std::min<u64>({1ull << kMaxLaunchLog2, target, split_cap}));
    const u64 rest = hi - cursor, nr = (rest + cap - 1) / cap;
    const u64 n = (rest + nr - 1) / nr;
    *cap_out = cap;
    return n;
}
static double old_rho(double rho, u64 mx, u64 newly_parked, u64 round_states) {
    rho = std::max(0.5 * rho, (double)(mx + newly_parked) / (double)round_states);
    return rho;
}

static int check_sizing(u64* levels, u64* rounds_total) {
    const u64 frontiers[] = {1, 1ull << 20, (1ull << 21) - 1, 1ull << 21, (1ull << 25) + 1, 300000000ull};
    const double rhos[] = {0.02, 0.5, 1, 7}, fills[] = {0.5, 2};
    const int splits[] = {1, 4};
    const u64 kcaps[] = {1ull << 20, 1ull << 23, 1ull << 25};  // keys_per_dest defaults at 64, 8 and 2 ranks
    for (u64 frontier : frontiers)
        for (double rho : rhos)
            for (double fill : fills)
                for (int split : splits)
                    for (u64 kcap : kcaps) {
                        const OldD D{split, fill};
                        const u64 sc = split_cap(frontier, split);
                        CHECK(sc == old_split_cap(frontier, D), "split_cap(%llu, %d)", (ull)frontier, split);
                        const u64 lo = 12345, hi = lo + frontier;
                        u64 cursor = lo, rounds = 0, least = ~0ull, most = 0;
                        while (cursor < hi) {
                            u64 cap = 0;
                            const u64 want = old_round(hi, cursor, kcap, rho, sc, D, &cap);
                            const u64 n = round_states(hi - cursor, kcap, fill, rho, sc, 1ull << kMaxLaunchLog2);
                            CHECK(n == want, "round_states: frontier %llu rho %g fill %g split %d kcap %llu at %llu: %llu, the "
                                  "loop's expression gives %llu", (ull)frontier, rho, fill, split, (ull)kcap,
                                  (ull)(cursor - lo), (ull)n, (ull)want);
                            CHECK(n >= 1 && n <= cap && n <= hi - cursor, "a round of %llu states, cap %llu, rest %llu", (ull)n,
                                  (ull)cap, (ull)(hi - cursor));
                            least = std::min(least, n);
                            most = std::max(most, n);
                            cursor += n;
                            ++rounds;
                        }
                        CHECK(cursor == hi, "the rounds sum to %llu, the frontier is %llu", (ull)(cursor - lo), (ull)frontier);
                        CHECK(frontier < (1ull << 21) || rounds >= (u64)split, "frontier %llu in %llu rounds, split %d",
                              (ull)frontier, (ull)rounds, split);
                        CHECK(most - least <= 1, "frontier %llu rho %g fill %g split %d kcap %llu: rounds of %llu to %llu states",
                              (ull)frontier, rho, fill, split, (ull)kcap, (ull)least, (ull)most);
                        ++*levels;
                        *rounds_total += rounds;
                    }
    const u64 mxs[] = {0, 1, 1000, 1ull << 25}, parks[] = {0, 3, 1ull << 20}, states[] = {1, 77, 1ull << 25};
    for (double rho : rhos)
        for (u64 mx : mxs)
            for (u64 pk : parks)
                for (u64 st : states)
                    CHECK(next_rho(rho, mx, pk, st) == old_rho(rho, mx, pk, st), "next_rho(%g, %llu, %llu, %llu)", rho, (ull)mx,
                          (ull)pk, (ull)st);
    return 0;
}

// ---- the set epoch: the `if` of the two run starts before it became next_set_epoch
static void old_epoch(uint32_t* set_epoch, bool* cleared, uint32_t ep_max, bool tagged_by_caller) {
    const bool tagged = ep_max > 0 && tagged_by_caller;
    *cleared = false;
    if (tagged && *set_epoch >= 1 && *set_epoch < ep_max) {
        *set_epoch += 1;
    } else {
        *cleared = true;
        *set_epoch = tagged ? 1 : 0;
    }
}

static int check_epochs() {
    const uint32_t ep_maxes[] = {0, 1, 2, 255};
    for (uint32_t cur = 0; cur <= 255; ++cur)
        for (uint32_t ep_max : ep_maxes)
            for (int tagged = 0; tagged < 2; ++tagged) {
                uint32_t e = cur;
                bool cleared = false;
                old_epoch(&e, &cleared, ep_max, tagged != 0);
                const SetEpoch got = next_set_epoch(cur, ep_max, tagged != 0);
                CHECK(got.epoch == e && got.clear == cleared, "next_set_epoch(%u, %u, %d) = (%u, %d), the old if (%u, %d)", cur,
                      ep_max, tagged, got.epoch, got.clear, e, cleared);
                CHECK(got.epoch <= ep_max, "epoch %u above ep_max %u", got.epoch, ep_max);
                CHECK(got.epoch > 1 || got.clear, "epoch %u without a clear (from %u)", got.epoch, cur);
                CHECK(tagged || (got.epoch == 0 && got.clear), "an untagged run at epoch %u", got.epoch);
            }
    return 0;
}

int main() {
    const int worlds[] = {1, 2, 3, 8, kPlanMaxWorld};
    int rounds = 0;
    for (int W : worlds)
        for (int trial = 0; trial < 12; ++trial) {
            const u64 kcap = trial % 2 ? 64 : 1000, ovf_cap = trial % 3 ? 5000 : 10;
            if (play_round(W, kcap, ovf_cap, trial)) return 1;
            ++rounds;
        }
    u64 levels = 0, sized = 0;
    if (check_sizing(&levels, &sized)) return 1;
    if (check_epochs()) return 1;
    printf("ok %d exchange rounds over 5 worlds, %llu levels in %llu sized rounds, 2048 epoch cases\n", rounds, (ull)levels,
           (ull)sized);
    return 0;
}
