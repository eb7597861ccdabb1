// ring_admit_check.cpp — a host model of the ring's device-side admission (rmc_plan.h
// admit_*, rmc_units.h): W waves run the claim protocol of expand_body's dynamic units
// in random interleavings and the host loop of rmc_run_bfs re-launches what stopped.
//
// A wave: claim — the next unit, or with the stop bit raised nothing (the count is taken
// back); walk the unit's states, each yielding 0..bound new ones into its list; flush the
// list into the count before it could pass list_cap, and when that takes the count past
// the stop raise the stop bit — a step of its own, so other waves claim between the two;
// claim again.  A wave that claims nothing flushes and leaves.  The model's list is
// flushed as late as it can be, so a wave carries up to list_cap entries into a unit.
//
// Checked on every run: the count never passes live_lo + win; every unit is claimed
// exactly once over the re-launches; the live_lo a re-launch takes from wnext passes
// no unfinished state; a re-launch progresses or ends in the too-small verdict; a
// window with room for the whole bound never stops, one below the reserve never starts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rmc_plan.h"
#include "rmc_units.h"

using namespace rmc_host;
typedef uint64_t u64;
typedef uint32_t u32;

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

static int fails = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (fails++ < 20) {                  \
                printf("FAIL %s: ", #cond);      \
                printf(__VA_ARGS__);             \
                printf("\n");                    \
            }                                    \
        }                                        \
    } while (0)

enum Yield { kNone, kAll, kRandom, kSparse };  // kSparse: the bound once in `bound` states, about 1 on average
enum Verdict { kDone, kTooSmall, kNoFit };
constexpr u64 kListCap = 512;  // rmc_dev_state.h WCAP

struct Wave {
    int pc = 1;        // 1: to claim, 2: in a unit, 3: left
    bool raise = false;  // a flush took the count past the stop: the stop bit is raised next
    u64 list = 0;      // listed new states not yet in the count
    std::vector<u64> todo;  // the unit's states still to walk
};

struct Run {
    u64 lo, nf, win, bound, W;
    u32 wt, ut;
    Yield yield;
    // the device
    u64 count = 0, wnext = 0, stop = 0, lim = 0, live_lo = 0;
    std::vector<uint8_t> claimed, done;  // per unit, per state of the launch
    u64 launches = 0, stops = 0;

    void flush(Wave& w) {
        if (!w.list) return;
        CHECK(count + w.list <= lim, "a flush reaches %llu, limit %llu", (unsigned long long)(count + w.list),
              (unsigned long long)lim);
        count += w.list;
        if (count > stop) w.raise = true;
        CHECK(count <= live_lo + win, "count %llu passes live_lo + win = %llu", (unsigned long long)count,
              (unsigned long long)(live_lo + win));
        w.list = 0;
    }

    void step(Wave& w) {
        const u32 ng = rmc_units::unit_groups(wt, ut);
        if (w.raise) {  // (one lane's atomics on one word: before the wave's next claim)
            wnext |= rmc_units::kStopBit;
            w.raise = false;
        } else if (w.pc == 1) {
            const u32 id = (u32)wnext++;
            if (id & rmc_units::kStopBit) wnext += 0xFFFFFFFFull;  // not a claim: taken back
            const rmc_units::Unit un = rmc_units::unit_decode(id, wt, ut, ng);
            if (un.win >= nf) {  // past the launch, or nothing admitted: the wave leaves
                if (id & rmc_units::kStopBit) ++stops;
                flush(w);
                w.raise = false;  // (raised or not, it claims nothing more)
                w.pc = 3;
                return;
            }
            CHECK(id < claimed.size() && !claimed[id], "unit %u claimed twice", id);
            if (id < claimed.size()) claimed[id] = 1;
            const u64 wn = std::min<u64>(nf - un.win, 256ull * wt);
            w.todo.clear();
            for (u32 t = un.tile0; t < un.tile0 + un.ntiles; ++t)
                for (u32 l = 0; l < 64; ++l) {
                    const u64 p = (u64)t * 256 + un.quarter * 64 + l;
                    if (p < wn) w.todo.push_back(un.win + p);
                }
            CHECK(w.todo.size() <= unit_states(wt, ut), "a unit of %zu states", w.todo.size());
            w.pc = 2;
        } else if (w.pc == 2) {
            if (w.todo.empty()) {
                w.pc = 1;
                return;
            }
            const u64 s = w.todo.back();
            w.todo.pop_back();
            CHECK(lo + s >= live_lo, "state %llu below live_lo %llu is read", (unsigned long long)(lo + s),
                  (unsigned long long)live_lo);
            const u64 y = yield == kNone     ? 0
                          : yield == kAll    ? bound
                          : yield == kRandom ? rnd() % (bound + 1)
                                             : (rnd() % bound == 0 ? bound : 0);
            if (w.list + y > kListCap) flush(w);
            w.list += y;
            CHECK(!done[s], "state %llu walked twice", (unsigned long long)s);
            done[s] = 1;
        }
    }

    // One launch: every wave to its end, in a random interleaving with bursts.
    void launch() {
        ++launches;
        std::vector<Wave> waves(W);
        u64 left = W;
        while (left) {
            Wave& w = waves[rnd() % W];
            if (w.pc == 3) continue;
            // a burst: this wave runs ahead while the others sit on old reads
            u64 burst = rnd() % 4 == 0 ? 1 + rnd() % 2000 : 1;
            while (burst-- && w.pc != 3) step(w);
            if (w.pc == 3) --left;
        }
    }

    Verdict run() {
        const u32 ng = rmc_units::unit_groups(wt, ut);
        const u64 total = rmc_units::units_total(nf, wt, ut);
        claimed.assign(total, 0);
        done.assign(nf, 0);
        count = lo + nf;  // the frontier is the newest level
        live_lo = lo;
        u64 reserve = admit_reserve(W, total, unit_states(wt, ut), bound, kListCap);
        if (!admit_fits(count, admit_stop(live_lo + win, reserve))) return kNoFit;
        for (;;) {
            stop = admit_stop(live_lo + win, reserve);
            lim = launch_store_limit(~0ull, true, live_lo, win);
            const u64 before = wnext, stops0 = stops;
            launch();
            CHECK((wnext >> 32) <= W, "%llu waves left on the stop bit", (unsigned long long)(wnext >> 32));
            wnext = rmc_units::units_claimed(wnext);  // the host clears the stop bit and the leavers' count
            if (wnext >= total) break;
            CHECK(stops > stops0, "a launch ended short of its units without an admission stop");
            CHECK(wnext > before, "a re-launch claimed nothing");
            const u64 nl = admit_live_lo(lo, nf, wnext, wt, 4ull * ng);
            CHECK(nl >= live_lo && nl <= lo + nf, "live_lo %llu", (unsigned long long)nl);
            for (u64 s = 0; s < nl - lo; ++s)
                if (!done[s]) {
                    CHECK(false, "live_lo %llu passes the unfinished state %llu", (unsigned long long)nl,
                          (unsigned long long)(lo + s));
                    break;
                }
            live_lo = nl;
            reserve = admit_reserve(W, total - wnext, unit_states(wt, ut), bound, kListCap);  // the units left
            if (!admit_fits(count, admit_stop(live_lo + win, reserve))) return kTooSmall;
            if (launches > total + 2) {
                CHECK(false, "no end after %llu launches", (unsigned long long)launches);
                return kTooSmall;
            }
        }
        for (u64 id = 0; id < total; ++id) CHECK(claimed[id] == 1, "unit %llu never claimed", (unsigned long long)id);
        for (u64 s = 0; s < nf; ++s)
            if (!done[s]) {
                CHECK(false, "state %llu never walked", (unsigned long long)s);
                break;
            }
        return kDone;
    }
};

int main() {
    // the plan functions on their own
    CHECK(launch_window_tiles(1, 1024, 16) == 1 && launch_window_tiles(1024 * 256 * 3 + 1, 1024, 16) == 4 &&
              launch_window_tiles(1ull << 28, 1536, 16) == 16,
          "launch_window_tiles");
    CHECK(unit_states(16, 8) == 512 && unit_states(1, 8) == 64 && unit_states(16, 16) == 1024, "unit_states");
    CHECK(admit_reserve(6144, 1 << 19, 512, 30, 512) == 6144ull * (512 * 30 + 512) &&
              admit_reserve(6144, 3, 512, 30, 512) == 3ull * (512 * 30 + 512),
          "admit_reserve");
    CHECK(admit_stop(150, 200) == 0 && admit_stop(600, 200) == 400, "admit_stop");
    CHECK(!admit_fits(400, 400) && admit_fits(399, 400) && !admit_fits(0, 0), "admit_fits");
    CHECK(admit_live_lo(1000, 5000, 7, 2, 8) == 1000 && admit_live_lo(1000, 5000, 17, 2, 8) == 1000 + 2 * 512 &&
              admit_live_lo(1000, 700, 100, 2, 8) == 1700,
          "admit_live_lo");
    CHECK(admit_needs_reserve(31, 10, 20) && !admit_needs_reserve(30, 10, 20), "admit_needs_reserve");
    CHECK(launch_store_limit(900, false, 10, 20) == 900 && launch_store_limit(900, true, 10, 20) == 30 &&
              launch_store_limit(25, true, 10, 20) == 25,
          "launch_store_limit");

    u64 cases = 0, done = 0, small = 0, nofit = 0, relaunched = 0;
    const u64 Ws[] = {1, 4, 64}, bounds[] = {30, 52};
    const u32 shapes[][2] = {{1, 8}, {16, 8}};  // (wt, ut): units of 64 and of 512 states
    for (u64 W : Ws)
        for (auto& sh : shapes)
            for (u64 bound : bounds)
                for (int y = 0; y < 4; ++y) {
                    const u32 wt = sh[0], ut = sh[1];
                    // more windows than the waves claim at once, and a last one cut short
                    const u64 nf = (12 + W) * 256 * wt + 100, lo = 5000;
                    const u64 reserve = admit_reserve(W, ~0ull, unit_states(wt, ut), bound, kListCap);
                    // from "the reserve does not fit" up to "never stops"
                    const u64 wins[] = {reserve / 2,
                                        reserve + nf,  // stop = count: the last window that does not fit
                                        reserve + nf + 1,
                                        reserve + nf + 64,
                                        reserve + nf + nf / 2,
                                        reserve + 2 * nf,
                                        reserve + nf + nf * bound / 2,
                                        nf + nf * bound + reserve};
                    for (size_t wi = 0; wi < sizeof wins / sizeof *wins; ++wi)
                        for (int seed = 0; seed < 3; ++seed) {
                            Run r{};
                            r.lo = lo, r.nf = nf, r.win = wins[wi], r.bound = bound, r.W = W, r.wt = wt, r.ut = ut;
                            r.yield = (Yield)y;
                            const Verdict v = r.run();
                            ++cases;
                            done += v == kDone;
                            small += v == kTooSmall;
                            nofit += v == kNoFit;
                            relaunched += v == kDone && r.launches > 1;
                            if (wi <= 1) CHECK(v == kNoFit, "window %llu starts", (unsigned long long)wins[wi]);
                            if (wi >= 2) CHECK(v != kNoFit, "window %llu does not start", (unsigned long long)wins[wi]);
                            if (wi == 7)
                                CHECK(v == kDone && r.launches == 1 && r.stops == 0, "the widest window stopped (%llu launches)",
                                      (unsigned long long)r.launches);
                            // about one new state per state into room for half a level: it stops
                            if (y == kSparse && wi == 4) CHECK(r.stops > 0, "no stop in a window of 1.5 levels");
                            if (y == kNone && wi >= 2) CHECK(v == kDone && r.launches == 1, "no yield, yet a stop");
                        }
                }
    CHECK(relaunched > 0 && small > 0 && done > 0 && nofit > 0, "the sweep misses a regime");
    printf("%s %llu cases, %llu completed (%llu over re-launches), %llu too small, %llu reserve does not fit\n",
           fails ? "FAILED" : "ok", (unsigned long long)cases, (unsigned long long)done, (unsigned long long)relaunched, (unsigned long long)small,
           (unsigned long long)nofit);
    if (fails) printf("%d checks failed\n", fails);
    return fails ? 1 : 0;
}
